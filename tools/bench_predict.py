#!/usr/bin/env python3
"""Time the mask / validation-count path that works from the low-resolution logits (ops.seg_predict, CAVP.predict_lowres,
MIoU / ForegroundDetect.update_lowres) against the full-resolution path it replaces.  B = 32 at 224x224:

  * kernel rows, C = 2, 24, 71: seg_predict (a) mask only, (b) confusion counts only, next to the old launches for the same
    result (bilinear_to_nchw, seg_confusion on its output, torch argmax);
  * graph rows: config #1's eval forward (bf16) captured twice in one process,
      old: model(image, audio, eval_mode=True) + MIoU.update + ForegroundDetect.update
      new: model.predict_lowres(image, audio) + the two update_lowres
    and replayed alternately in `--repeats` windows of `--iters` replays each: per path the median window and the spread
    (max - min over the windows) of ms per replay.  The counts of the two graphs are compared before anything is timed.

Prints one JSON line per row; --jsonl appends them to a file.

usage: python tools/bench_predict.py [--iters 50] [--repeats 7] [--no-model] [--jsonl profiles/seg_predict_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cavp_amd import metrics as MT  # noqa: E402
from cavp_amd import ops  # noqa: E402

DEV = "cuda:0"
ROWS = []


def report(name, **fields):
    row = {"item": name, **fields}
    ROWS.append(row)
    print(json.dumps(row), flush=True)


def gpu_time(fn, iters, warmup=3):
    """Mean device time per call (microseconds) from events around `iters` back-to-back calls."""
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


def bench_kernels(iters, B=32, hw=(224, 224)):
    g = torch.Generator(device="cpu").manual_seed(0)
    H, W = hw
    for C in (2, 24, 71):
        for dtype in (torch.bfloat16, torch.float32):
            lo = (torch.randn(B, H // 4, W // 4, C, generator=g) * 4).to(dtype).to(DEV)
            full = torch.empty((B, C, H, W), dtype=torch.float32, device=DEV)
            ops.bilinear_to_nchw(lo, full, False)
            y = torch.randint(0, C, (B, H, W), generator=g)
            y[:, :, :16] = 255
            y = y.to(DEV)
            y = torch.where(torch.rand(y.shape, generator=g).to(DEV) < 0.8, full.argmax(1), y)   # a realistic hot bin
            mask = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
            M = torch.zeros((C + 1) * C, dtype=torch.int64, device=DEV)
            Mref = torch.zeros_like(M)
            ops.seg_predict(lo, hw, mask=mask, labels=y, num_classes=C, ignore=255, M=M)
            ops.seg_confusion(full, y, C, 255, Mref)
            if not (torch.equal(mask.long(), full.argmax(1)) and torch.equal(M, Mref)):
                raise SystemExit(f"seg_predict differs from the full-resolution path at C={C} {dtype}")
            tag = f"B{B} C{C} {str(dtype).split('.')[-1]} {H}x{W}"
            lo_b, lab_b, full_b = lo.numel() * lo.element_size(), y.numel() * 8, full.numel() * 4
            us = gpu_time(lambda: ops.seg_predict(lo, hw, mask=mask), iters)
            report(f"kernel seg_predict mask only {tag}", us=round(us, 2), bytes=lo_b + mask.numel())
            us = gpu_time(lambda: ops.seg_predict(lo, hw, labels=y, num_classes=C, ignore=255, M=M), iters)
            report(f"kernel seg_predict confusion only {tag}", us=round(us, 2), bytes=lo_b + lab_b)
            us_up = gpu_time(lambda: ops.bilinear_to_nchw(lo, full, False), iters)
            us_cf = gpu_time(lambda: ops.seg_confusion(full, y, C, 255, M), iters)
            us_am = gpu_time(lambda: full.argmax(1), max(5, iters // 5))
            report(f"old path {tag}", bilinear_to_nchw_us=round(us_up, 2), seg_confusion_us=round(us_cf, 2),
                   torch_argmax_us=round(us_am, 2), full_res_MB=round(full_b / 1e6, 1))
            del lo, full, y, mask


def capture(step):
    from cavp_amd.train import _no_gc_during_capture
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
    return graph


def bench_graphs(iters, repeats, B=32, hw=(224, 224)):
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_inputs, synth_state_dict
    C, K = 22, 24
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, True, True], audio_backbone="vgg",
                                 num_classes=C, batch_size=B, local_rank="cpu")
    m = CAVP(50, None, num_classes=C, args=args)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.eval().to(DEV).set_compute_dtype(torch.bfloat16)
    image, audio, _ = synth_inputs(B, hw, num_classes=C, seed=5)
    image, audio = image.to(DEV), audio.to(DEV)
    label = torch.randint(0, K, (B,) + hw, generator=torch.Generator().manual_seed(9)).to(DEV)
    acc = {p: (MT.MIoU(K, 255, 0), MT.ForegroundDetect(K)) for p in ("old", "new")}

    def old():
        o, _, _ = m(image, audio, eval_mode=True)
        acc["old"][0].update(o, label)
        acc["old"][1].update(o, label)

    def new():
        lo = m.predict_lowres(image, audio)
        acc["new"][0].update_lowres(lo, label)
        acc["new"][1].update_lowres(lo, label)

    with torch.no_grad():
        graphs = {"old": capture(old), "new": capture(new)}
    for p in graphs:
        for a in acc[p]:
            a.reset()
        graphs[p].replay()
    torch.cuda.synchronize()
    if not all(torch.equal(a.counts(), b.counts()) for a, b in zip(acc["old"], acc["new"])):
        raise SystemExit("the two graphs count differently")
    for p in graphs:   # warm both before the first timed window
        for _ in range(5):
            graphs[p].replay()
    torch.cuda.synchronize()
    ms = {"old": [], "new": []}
    for _ in range(repeats):
        for p in ("old", "new"):
            ms[p].append(gpu_time(graphs[p].replay, iters, warmup=1) / 1e3)
    for p, what in (("old", "eval forward + MIoU.update + ForegroundDetect.update"), ("new", "predict_lowres + 2 x update_lowres")):
        v = ms[p]
        report(f"graph {p}: {what}, B{B} C{C} K{K} bf16", ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4),
               ms_max=round(max(v), 4), spread_ms=round(max(v) - min(v), 4), windows=repeats, replays_per_window=iters)
    report("graph new - old", delta_ms_median=round(statistics.median(ms["new"]) - statistics.median(ms["old"]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--jsonl", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict needs the GPU: there is nothing to time without one")
    from cavp_amd.hostinfo import cap_torch_threads
    cap_torch_threads()
    bench_kernels(a.iters)
    if not a.no_model:
        bench_graphs(a.iters, a.repeats)
    if a.jsonl:
        with open(a.jsonl, "a") as f:
            for row in ROWS:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
