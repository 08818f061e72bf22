#!/usr/bin/env python3
"""Generate tests/golden/videoval.npz by running the REFERENCE's own functions (read-only import from /root/reference) through the
validation loop of its AVSBench object trainer (trainer/trainer_cavp_avs_obj.py:292-363) on the CPU: per video MIoU /
ForegroundDetect on every frame's logits, mask_iou(argmax(vid_pred), labels), Eval_Fmeasure(softmax(vid_pred)[:, 1], labels), the
two AverageMeters, the rounding of lines 349-352 and get_performance.

Authoring-container only, like tools/make_golden_metrics.py (the same import recipe: the stub packages of tools/_shims, Tensor.cuda
patched to the identity): /root/reference does not exist on the GPU box.

Two cases, each 4 videos x T = 5 frames, C = K = 2: "vec" at 24 x 28 (HW % 4 == 0: the vector path) and "sca" at 7 x 9 (the
scalar path).  Video 1 has one frame with an all-zero gt (skipped by Eval_Fmeasure, background overlap in mask_iou); the gt of
video 2 is all zero (F = 0, J from the background overlap).

A condition on the INPUTS, asserted before writing: the float64 softmax of channel 1 lies at least 1e-5 from every threshold of
linspace(0, 1 - 1e-10, 255) at every pixel (offending pixels are redrawn), so the last-bit differences between one float32 expf
and another cannot move a pixel across a threshold: the integer counts of the fixture hold for every faithful float32 softmax.
Also asserted: both means lie at least 1e-5 from a 4-decimal rounding boundary.

Stored per case: logits f32 [4, 5, 2, H, W], labels int64 [4, 5, H, W]; the reference's per-video J (float32) and F (float64, the
Python floats), the two unrounded means and the rounded pair, the 5-tuple of get_performance; and the integer counts of every frame
(mask_iou sums [20, 4], F-measure histograms [20, 2, 256], the (K+1) x K confusion counts) from the float64 softmax.

usage: python tools/make_golden_videoval.py [--out tests/golden]
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "_shims"), "/root/reference", REPO]

import numpy  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
import utils.avsbench_utils as AU  # noqa: E402
import utils.eval_utils as EU  # noqa: E402
from utils.avsbench_pyutils import AverageMeter  # noqa: E402

B, T, K, PR = 4, 5, 2, 255
MARGIN = 1e-5


def softmax1_f64(x):
    """float64 softmax of channel 1 of [..., 2, H, W] float32 logits."""
    d = x.astype(np.float64)
    m = d.max(-3, keepdims=True)
    e = np.exp(d - m)
    return e[..., 1, :, :] / e.sum(-3)


def draw_logits(rs, shape, th64):
    """float32 logits whose float64 channel-1 softmax keeps MARGIN from every threshold: offending pixels are redrawn."""
    x = (rs.randn(*shape) * 2).astype(np.float32)
    for _ in range(100):
        p = softmax1_f64(x)
        near = np.abs(p[..., None] - th64).min(-1) < MARGIN
        if not near.any():
            return x
        idx = np.argwhere(near)
        for c in range(shape[-3]):
            x[(*idx[:, :-2].T, c, idx[:, -2], idx[:, -1])] = (rs.randn(len(idx)) * 2).astype(np.float32)
    raise AssertionError("could not draw logits away from the thresholds")


def rounding_margin(v):
    """Distance of v from the nearest 4-decimal rounding boundary (k + 0.5) * 1e-4."""
    s = v * 1e4
    return abs(s - np.floor(s) - 0.5) * 1e-4


def case(out, name, rs, hw):
    H, W = hw
    th = torch.linspace(0, 1 - 1e-10, PR)
    th64 = th.numpy().astype(np.float64)
    logits = draw_logits(rs, (B, T, K, H, W), th64)
    x = torch.from_numpy(logits)
    amax = x.argmax(2).numpy()
    labels = np.where(rs.rand(B, T, H, W) < 0.8, amax, rs.randint(0, 2, size=(B, T, H, W))).astype(np.int64)
    labels[1, 3] = 0        # one frame with an all-zero gt
    labels[2] = 0           # one video whose gt is all zero
    p64 = softmax1_f64(logits)
    assert np.abs(p64[..., None] - th64).min() >= MARGIN
    assert (np.sort(logits, axis=2)[:, :, 1] > np.sort(logits, axis=2)[:, :, 0]).all()          # no argmax ties

    # ---- the reference's loop (mask_num == T for every video) ----
    miou_measure = EU.MIoU(num_classes=K, ignore_index=255, local_rank=0)
    fg_measure = EU.ForegroundDetect(num_classes=K, local_rank=0)
    avg_meter_miou, avg_meter_F = AverageMeter("miou"), AverageMeter("F_score")
    Js, Fs = [], []
    for b in range(B):
        pix_label = torch.from_numpy(labels[b:b + 1].copy())[:, :, None]                        # [1, T, 1, H, W]
        pred_list = []
        for i in range(T):
            avl_map_logits = x[b, i, None]
            curr_pix_label = pix_label[0, i]
            fg_measure(avl_map_logits, curr_pix_label.clone())
            miou_measure(avl_map_logits, curr_pix_label.clone())                                # (writes -1 into its target)
            pred_list.append(avl_map_logits)
        vid_pred = torch.cat(pred_list)
        miou_i = AU.mask_iou(torch.argmax(vid_pred, dim=1), pix_label[0].squeeze(1))
        f_score_i = AU.Eval_Fmeasure(torch.softmax(vid_pred, dim=1)[:, 1, :, :], pix_label.float().squeeze())
        avg_meter_miou.add({"miou": miou_i})
        avg_meter_F.add({"F_score": f_score_i})
        Js.append(float(miou_i))
        Fs.append(f_score_i)
    avs_miou = avg_meter_miou.pop("miou").item()
    avs_f = avg_meter_F.pop("F_score")
    assert rounding_margin(avs_miou) >= MARGIN and rounding_margin(avs_f) >= MARGIN, (avs_miou, avs_f)
    assert Fs[2] == 0.0 and Js[2] > 0.0
    perf = EU.get_performance(miou_measure, fg_measure, class_list=None)

    # ---- the integer counts of every frame, from the float64 softmax ----
    p = amax.reshape(B * T, -1)
    t = labels.reshape(B * T, -1)
    bins = np.searchsorted(th64, p64.reshape(B * T, -1), side="right")
    stats = np.stack([(p * t).sum(1), np.maximum(p, t).sum(1), ((1 - t) * (1 - p)).sum(1), t.sum(1)], 1).astype(np.int64)
    hist = np.zeros((B * T, 2, PR + 1), dtype=np.int64)
    for n in range(B * T):
        hist[n, 0] = np.bincount(bins[n], minlength=PR + 1)
        hist[n, 1] = np.bincount(bins[n][t[n] != 0], minlength=PR + 1)
    M = np.bincount((t * K + p).ravel(), minlength=(K + 1) * K).reshape(K + 1, K).astype(np.int64)

    out[f"{name}_logits"] = logits
    out[f"{name}_labels"] = labels
    out[f"{name}_J"] = np.array(Js, dtype=np.float32)
    out[f"{name}_F"] = np.array(Fs, dtype=np.float64)
    out[f"{name}_means"] = np.array([avs_miou, avs_f], dtype=np.float64)
    out[f"{name}_rounded"] = np.array([numpy.round(avs_miou, 4), numpy.round(avs_f, 4)], dtype=np.float64)
    out[f"{name}_perf"] = np.array([float(v) for v in perf], dtype=np.float64)
    out[f"{name}_stats"] = stats
    out[f"{name}_hist"] = hist
    out[f"{name}_M"] = M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    out = {}
    case(out, "vec", np.random.RandomState(2024), (24, 28))      # (seeds under which the rounding-margin assertion holds)
    case(out, "sca", np.random.RandomState(2025), (7, 9))
    path = os.path.join(a.out, "videoval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
