#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz by running the REFERENCE metric code (read-only import of utils/eval_utils.py and
utils/avsbench_utils.py from /root/reference) on the CPU.

Authoring-container only, like tools/make_golden.py: /root/reference does not exist on the GPU box.  Import recipe: the stub
packages of tools/_shims (torchmetrics, which eval_utils imports at module scope; cv2 / torchvision for avsbench_utils), and
Tensor.cuda patched to the identity because ForegroundDetect.get_metric_results and _eval_pr call .cuda().

Inputs are stored as int8-quantised logits (value / 8: many exact ties) and int64 labels; the outputs are the reference's:
  vpo_*   K=24, C=22, B=3, 37x53, two accumulated batches (trainer_cavp_vpo_mono.py:253 shape): MIoU inter / union / correct /
          label and the rounded (miou, acc) after each call, ForegroundDetect confusion_matrix_ and rounded fdr / f1 / f0.3 with
          and without a class_list;
  avss_*  K=C=71, B=2, 32x48, one batch, the same outputs;
  avs_*   C=2, a 5-frame clip at 56x64 with one all-zero gt frame: mask_iou (int64 and float32 inputs), per-frame _eval_pr
          prec / recall, Eval_Fmeasure on a probability map that holds exact threshold values.
Also stored: the confusion counts M and the F-measure histograms as the integer restatement computes them (numpy), which the host
tests finalise.

usage: python tools/make_golden_metrics.py [--out tests/golden]
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "_shims"), "/root/reference", REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
import utils.avsbench_utils as AU  # noqa: E402
import utils.eval_utils as EU  # noqa: E402

CLASS_LIST_VPO = [0, 3, 5, 7, 11, 21, 23]
CLASS_LIST_AVSS = [0, 1, 2, 10, 40, 70]


def quant_logits(rs, shape):
    """int8 logits (value / 8 on use): small range -> many exact ties in the argmax."""
    q = rs.randint(-4, 5, size=shape).astype(np.int8)
    return q


def make_labels(rs, amax, K, extra):
    """Labels equal to the prediction for ~60 % of the pixels, random valid classes elsewhere, plus the special values `extra`."""
    lab = np.where(rs.rand(*amax.shape) < 0.6, amax, rs.randint(0, K, size=amax.shape)).astype(np.int64)
    sel = rs.rand(*amax.shape)
    edge = np.linspace(0.0, 0.15, len(extra) + 1)
    for i, v in enumerate(extra):
        lab[(sel >= edge[i]) & (sel < edge[i + 1])] = v
    return lab


def confusion(logits, labels, K, ignore):
    """Integer restatement: M[(K+1) x K], row t < K or K for t >= K; pixels with t >= 0 and t != ignore."""
    p = torch.from_numpy(logits).argmax(1).numpy().ravel()
    t = labels.ravel()
    ok = (t >= 0) & (t != ignore)
    row = np.where(t[ok] < K, t[ok], K)
    return np.bincount(row * K + p[ok], minlength=(K + 1) * K).reshape(K + 1, K).astype(np.int64)


def seg_case(out, name, rs, K, C, B, hw, batches, class_list):
    H, W = hw
    lq = np.stack([quant_logits(rs, (B, C, H, W)) for _ in range(batches)])
    labs = []
    for b in range(batches):
        amax = torch.from_numpy(lq[b].astype(np.float32) / 8).argmax(1).numpy()
        labs.append(make_labels(rs, amax, K, [255, -1, K, K + 1, K + 2]))
    labs = np.stack(labs)
    miou = EU.MIoU(num_classes=K, ignore_index=255, local_rank=0)
    fd = EU.ForegroundDetect(num_classes=K, local_rank=0)
    calls = []
    for b in range(batches):
        x = torch.from_numpy(lq[b].astype(np.float32) / 8)
        fd(x, torch.from_numpy(labs[b].copy()))
        calls.append([float(v) for v in miou(x, torch.from_numpy(labs[b].copy()))])
    cm = np.array(fd.confusion_matrix_)
    out[f"{name}_logits_q"] = lq
    out[f"{name}_labels"] = labs
    out[f"{name}_meta"] = np.array([K, C, B, H, W, batches], dtype=np.int64)
    out[f"{name}_M"] = sum(confusion(lq[b].astype(np.float32) / 8, labs[b], K, 255) for b in range(batches))
    out[f"{name}_miou_calls"] = np.array(calls, dtype=np.float64)
    out[f"{name}_inter"] = np.asarray(miou.inter, dtype=np.float64)
    out[f"{name}_union"] = np.asarray(miou.union, dtype=np.float64)
    out[f"{name}_correct"] = np.asarray(float(miou.correct))
    out[f"{name}_label"] = np.asarray(float(miou.label))
    out[f"{name}_miou_cl"] = np.array([float(v) for v in miou.get_metric_results(class_list)])
    out[f"{name}_class_list"] = np.array(class_list, dtype=np.int64)
    out[f"{name}_fd_cm"] = cm
    out[f"{name}_fd"] = np.array([float(v) for v in fd.get_metric_results()])
    fd.confusion_matrix_ = cm          # (the reference turned it into a tensor in get_metric_results)
    out[f"{name}_fd_cl"] = np.array([float(v) for v in fd.get_metric_results(class_list)])


def avs_case(out, rs, T=5, hw=(56, 64), pr_num=255):
    H, W = hw
    lq = quant_logits(rs, (T, 2, H, W))
    x = torch.from_numpy(lq.astype(np.float32) / 8)
    amax = x.argmax(1)
    lab = np.where(rs.rand(T, H, W) < 0.75, amax.numpy(), rs.randint(0, 2, size=(T, H, W))).astype(np.int64)
    lab[2] = 0                                             # an all-zero gt frame: skipped by Eval_Fmeasure
    th = torch.linspace(0, 1 - 1e-10, pr_num)
    prob = torch.round(torch.softmax(x, dim=1)[:, 1] * 1024) / 1024     # (k / 1024: exact, and the fixture compresses)
    sel = rs.rand(T, H, W)
    idx = rs.randint(0, pr_num, size=(T, H, W))
    prob[torch.from_numpy(sel < 0.2)] = th[torch.from_numpy(idx[sel < 0.2])]   # pixels exactly on a threshold
    prob[torch.from_numpy((sel >= 0.2) & (sel < 0.22))] = 0.0
    prob[torch.from_numpy((sel >= 0.22) & (sel < 0.24))] = 1.0
    labt = torch.from_numpy(lab)
    out["avs_logits_q"] = lq
    out["avs_labels"] = lab
    out["avs_prob"] = prob.numpy()
    out["avs_mask_iou"] = np.asarray(float(AU.mask_iou(amax, labt)), dtype=np.float32)
    out["avs_mask_iou_f32"] = np.asarray(float(AU.mask_iou(amax.float(), labt.float())), dtype=np.float32)
    precs, recs = [], []
    for i in range(T):
        p, r = AU._eval_pr(prob[i], labt[i].float(), pr_num)
        precs.append(p.numpy())
        recs.append(r.numpy())
    out["avs_prec"] = np.stack(precs)
    out["avs_recall"] = np.stack(recs)
    out["avs_fmeasure"] = np.asarray(AU.Eval_Fmeasure(prob, labt.float(), pr_num=pr_num), dtype=np.float64)
    # the histograms the kernel must produce: bin = #{i : th[i] <= p}, over all pixels and over gt != 0
    b = np.searchsorted(th.numpy(), prob.numpy().reshape(T, -1), side="right")
    hist = np.zeros((T, 2, pr_num + 1), dtype=np.int64)
    for i in range(T):
        hist[i, 0] = np.bincount(b[i], minlength=pr_num + 1)
        hist[i, 1] = np.bincount(b[i][lab[i].ravel() != 0], minlength=pr_num + 1)
    out["avs_hist"] = hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    rs = np.random.RandomState(1234)
    out = {}
    seg_case(out, "vpo", rs, K=24, C=22, B=3, hw=(37, 53), batches=2, class_list=CLASS_LIST_VPO)
    seg_case(out, "avss", rs, K=71, C=71, B=2, hw=(32, 48), batches=1, class_list=CLASS_LIST_AVSS)
    avs_case(out, rs)
    path = os.path.join(a.out, "metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
