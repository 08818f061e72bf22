#!/usr/bin/env python3
"""Time the validation metrics on the GPU (cavp_amd.metrics): each counting kernel, the metric classes, a plain torch-on-device
restatement of the reference's calls (utils/eval_utils.py, utils/avsbench_utils.py), and the eval forward with and without
MIoU.update + ForegroundDetect.update in one hipGraph.  Prints one line per item: microseconds per call and, for the kernels,
effective TB/s (bytes the kernel must read / time).  Shapes: B=32 at 224x224 for C = 2, 24, 71 (the trainers' validation
batches), a 5-frame clip for mask_iou / Eval_Fmeasure.

usage: python tools/bench_metrics.py [--iters 50] [--no-model] [--json out.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cavp_amd import metrics as MT  # noqa: E402
from cavp_amd import ops  # noqa: E402

DEV = "cuda:0"
ROWS = []


def report(name, us, nbytes=None, **extra):
    row = {"item": name, "us": round(us, 2)}
    if nbytes:
        row["TB_s"] = round(nbytes / us / 1e6, 3)
    row.update(extra)
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def gpu_time(fn, iters, warmup=3):
    """Mean device time per call from events around `iters` back-to-back calls (the stream stays busy: launch-bound calls show
    their launch cost)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def wall_time(fn, iters, warmup=2):
    """Host wall time per call including its own synchronisation (the end-to-end cost a trainer sees)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


# ---- torch-on-device restatements of the reference calls (what a user of our model runs today) --------------------------------
def ref_miou_call(out, target, K, ignore=255):
    target = target.clone()
    target[target == ignore] = -1
    _, predict = torch.max(out, 1)
    p, t = predict.int() + 1, target.int() + 1
    labeled = (t > 0).sum()
    correct = ((p == t) * (t > 0)).sum()
    p64, t64 = predict + 1, target + 1
    p64 = p64 * (t64 > 0).long()
    inter = p64 * (p64 == t64).long()
    ai = torch.histc(inter.float(), bins=K, max=K, min=1)
    ap = torch.histc(p64.float(), bins=K, max=K, min=1)
    al = torch.histc(t64.float(), bins=K, max=K, min=1)
    return correct.cpu().numpy(), labeled.cpu().numpy(), ai.cpu().numpy(), (ap + al - ai).cpu().numpy()


def ref_fd_call(out, target, K, ignore=255):
    pred = torch.argmax(out, dim=1).squeeze().cpu().numpy()
    lab = target.squeeze().cpu().numpy()
    cm = np.zeros((K, K))
    for lt, lp in zip(lab, pred):
        lt, lp = lt.flatten(), lp.flatten()
        m = (lt >= 0) & (lt < K) & (lt != ignore)
        cm += np.bincount(K * lt[m].astype(int) + lp[m], minlength=K * K).reshape(K, K)
    return cm


def ref_mask_iou(pred, target, eps=1e-7):
    n, npix = pred.size(0), pred.size(-1) * pred.size(-2)
    empty = target.sum(dim=(1, 2)) == 0
    inter = (pred * target).sum(dim=(1, 2))
    union = torch.maximum(pred, target).sum(dim=(1, 2))
    bg = ((1 - target) * (1 - pred)).sum(dim=(1, 2))
    inter[empty] = bg[empty]
    union[empty] = npix
    return torch.sum(inter / (union + eps)) / n


def ref_fmeasure(pred, gt, pr_num=255, beta2=0.3):
    th = torch.linspace(0, 1 - 1e-10, pr_num).to(pred.device)
    total, count, score = 0.0, 0, torch.zeros(pr_num)
    for i in range(pred.size(0)):
        if torch.mean(gt[i]) == 0.0:
            continue
        prec, recall = torch.zeros(pr_num, device=pred.device), torch.zeros(pr_num, device=pred.device)
        for j in range(pr_num):
            above = (pred[i] >= th[j]).float()
            tp = (above * gt[i]).sum()
            prec[j], recall[j] = tp / (above.sum() + 1e-20), tp / (gt[i].sum() + 1e-20)
        f = (1 + beta2) * prec * recall / (beta2 * prec + recall)
        f[f != f] = 0
        total += f
        count += 1
        score = total / count
    best = score.max()
    return best.item()


def bench_seg(iters, B=32, hw=(224, 224)):
    g = torch.Generator(device="cpu").manual_seed(0)
    for C, K in ((2, 2), (24, 24), (71, 71)):
        x = torch.randn(B, C, *hw, generator=g).to(DEV)
        y = torch.randint(0, K, (B, *hw), generator=g)
        y[:, :, :16] = 255
        y = y.to(DEV)
        # a realistic hot bin: most labels equal the prediction
        p = x.argmax(1)
        y = torch.where(torch.rand(y.shape, generator=g).to(DEV) < 0.8, p, y)
        nbytes = x.numel() * 4 + y.numel() * 8
        M = torch.zeros((K + 1) * K, dtype=torch.int64, device=DEV)
        us = gpu_time(lambda: ops.seg_confusion(x, y, K, 255, M), iters)
        report(f"kernel seg_confusion B{B} C{C} K{K} 224^2", us, nbytes, logits_MB=round(x.numel() * 4 / 1e6, 1))
        xu = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x)
        xu.copy_(x)
        us = gpu_time(lambda: ops.seg_confusion(xu, y, K, 255, M), iters)
        report(f"kernel seg_confusion B{B} C{C} K{K} 224^2 unaligned view (scalar path)", us, nbytes)
        m, f = MT.MIoU(K, 255, 0), MT.ForegroundDetect(K)
        report(f"MIoU.update+ForegroundDetect.update C{C}", gpu_time(lambda: (m.update(x, y), f.update(x, y)), iters))
        report(f"MIoU.__call__ C{C} (host sync, end to end)", wall_time(lambda: m(x, y), iters))
        report(f"ForegroundDetect.__call__ C{C} (end to end)", wall_time(lambda: (f(x, y), torch.cuda.synchronize()), iters))
        report(f"ForegroundDetect.get_metric_results C{C}", wall_time(lambda: f.get_metric_results(), iters))
        report(f"reference-style MIoU.__call__ C{C} (torch on device)", wall_time(lambda: ref_miou_call(x, y, K), max(3, iters // 5)))
        report(f"reference-style ForegroundDetect.__call__ C{C} (host bincount)", wall_time(lambda: ref_fd_call(x, y, K), 3, warmup=1))
        del x, xu, y


def bench_avs(iters, T=5, hw=(224, 224)):
    g = torch.Generator(device="cpu").manual_seed(1)
    logits = (torch.randn(T, 2, *hw, generator=g) * 2).to(DEV)
    gt = (torch.rand(T, *hw, generator=g) < 0.3).float().to(DEV)
    prob = torch.softmax(logits, 1)[:, 1].contiguous()
    pred = logits.argmax(1)
    st = torch.zeros((T, 4), dtype=torch.int64, device=DEV)
    report(f"kernel mask_iou_stats T{T} 224^2 int64/f32", gpu_time(lambda: ops.mask_iou_stats(pred, gt, st), iters), pred.numel() * 12)
    th = MT.thresholds(255, DEV)
    h = torch.zeros((T, 2, 256), dtype=torch.int32, device=DEV)
    report(f"kernel fmeasure_hist T{T} 224^2 probabilities", gpu_time(lambda: ops.fmeasure_hist(prob, gt, th, h), iters), prob.numel() * 8)
    report(f"kernel fmeasure_hist T{T} 224^2 logits (softmax in kernel)", gpu_time(lambda: ops.fmeasure_hist(logits, gt, th, h), iters),
           logits.numel() * 4 + gt.numel() * 4)
    report("mask_iou (device tensor, stream time)", gpu_time(lambda: MT.mask_iou(pred, gt), iters))
    report("mask_iou + .item() (end to end)", wall_time(lambda: MT.mask_iou(pred, gt).item(), iters))
    report("fmeasure_curve (stream time)", gpu_time(lambda: MT.fmeasure_curve(prob, gt), iters))
    report("Eval_Fmeasure (end to end)", wall_time(lambda: MT.Eval_Fmeasure(prob, gt), iters))
    report("Eval_Fmeasure on logits (end to end)", wall_time(lambda: MT.Eval_Fmeasure(logits, gt), iters))
    report("reference-style mask_iou + .item() (torch on device)", wall_time(lambda: ref_mask_iou(pred, gt).item(), iters))
    report("reference-style Eval_Fmeasure (torch on device)", wall_time(lambda: ref_fmeasure(prob, gt), 2, warmup=1))


def bench_graph(iters, B=32, hw=(224, 224)):
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_inputs, synth_state_dict
    from cavp_amd.train import _no_gc_during_capture
    C = 22
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, True, True], audio_backbone="vgg",
                                 num_classes=C, batch_size=B, local_rank="cpu")
    m = CAVP(50, None, num_classes=C, args=args)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.eval().to(DEV).set_compute_dtype(torch.bfloat16)
    image, audio, _ = synth_inputs(B, hw, num_classes=C, seed=5)
    image, audio = image.to(DEV), audio.to(DEV)
    label = torch.randint(0, 24, (B,) + hw).to(DEV)
    miou, fd = MT.MIoU(24, 255, 0), MT.ForegroundDetect(24)
    res = {}
    with torch.no_grad():
        for with_metrics in (False, True):
            def step():
                o, _, _ = m(image, audio, eval_mode=True)
                if with_metrics:
                    miou.update(o, label)
                    fd.update(o, label)
            step()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
                step()
            res[with_metrics] = gpu_time(graph.replay, iters)
            del graph
    report(f"eval forward B{B} C{C} bf16, one graph", res[False])
    report(f"eval forward + MIoU.update + ForegroundDetect.update, one graph", res[True], delta_us=round(res[True] - res[False], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    bench_seg(a.iters)
    bench_avs(a.iters)
    if not a.no_model:
        bench_graph(a.iters)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(ROWS, f, indent=1)


if __name__ == "__main__":
    main()
