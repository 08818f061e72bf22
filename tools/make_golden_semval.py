#!/usr/bin/env python3
"""Generate tests/golden/semval.npz by running the REFERENCE's own calc_color_miou_fscore, calc_color_miou and calc_binary_miou
(utils/avsbench_metrics.py, read-only import from /root/reference) on the CPU.

Authoring-container only, like tools/make_golden_videoval.py (the same import recipe: the stub packages of tools/_shims):
/root/reference does not exist on the GPU box.

Two cases of 2 clips x T = 3 frames: "vec" with K = 5 at 24 x 28 (HW % 4 == 0: the vector path) and "sca" with K = 3 at 7 x 9 (the
scalar path).  Each case is given to the reference in ONE call (all 6 frames) and in TWO calls (clip 0, clip 1) whose results are
added as the benchmark driver adds them (`ious += _ious`, float32).  The frames contain labels 255, -1 and K + 2 (>= K, not 255),
frame (0, 1) is all background in label and prediction, class K - 1 is never predicted, and frame (1, 2) has an empty foreground
(label 0 everywhere) under a prediction that has some.

Conditions asserted before writing: no argmax ties (the top-2 logit gap exceeds 1e-3 at every pixel), and every stored mean
(frame_miou, the binary value) that is not NaN is at least 1e-5: the tests compare them within 4 float32 ulp of the stored value, a
bound that would mean nothing at 0.

Stored per case (arrays only): logits f32 [2, 3, K, H, W], labels int64 [2, 3, H, W]; counts int64 [6, 3K + 4] (inter | pred | lab |
the four binary sums per frame, from a float64 argmax); and for the one-call run and each of the two calls the reference's four
outputs (ious, fscores, cls_count f32 [K], vid_miou_list f32 [frames]), calc_color_miou's two, and calc_binary_miou's value.

usage: python tools/make_golden_semval.py [--out tests/golden]
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
import utils.avsbench_metrics as AM  # noqa: E402

B, T = 2, 3
MARGIN = 1e-5


def draw(rs, K, hw):
    H, W = hw
    x = (rs.randn(B, T, K, H, W) * 2).astype(np.float32)
    x[:, :, K - 1] = x[:, :, :K - 1].min(2) - 1.0                     # class K - 1 is never predicted
    x[0, 1, 0] = x[0, 1, 1:].max(0) + 1.0                              # frame (0, 1): background everywhere
    for _ in range(100):                                               # no argmax ties: redraw pixels with a small top-2 gap
        top = np.sort(x, axis=2)
        near = top[:, :, -1] - top[:, :, -2] <= 1e-3
        if not near.any():
            break
        b, t, h, w = np.nonzero(near)
        x[b, t, :K - 1, h, w] = (rs.randn(len(b), K - 1) * 2).astype(np.float32)
    amax = x.astype(np.float64).argmax(2)
    labels = np.where(rs.rand(B, T, H, W) < 0.7, amax, rs.randint(0, K, size=(B, T, H, W))).astype(np.int64)
    labels[0, 1] = 0
    labels[1, 2] = 0                                                   # an empty foreground under a prediction that has some
    labels[0, 0, 0, :3] = [255, -1, K + 2]
    labels[1, 0, 1, :3] = [K + 2, 255, -1]
    labels[1, 1, 2, 0] = K - 1                                         # the class that is never predicted occurs as a label
    return x, labels, amax


def counts_f64(amax, labels, K):
    N = B * T
    p, l = amax.reshape(N, -1), labels.reshape(N, -1)
    out = np.zeros((N, 3 * K + 4), dtype=np.int64)
    for n in range(N):
        seen = l[n] >= 0
        ok = seen & (l[n] < K)
        out[n, :K] = np.bincount(p[n][ok & (p[n] == l[n])], minlength=K)
        out[n, K:2 * K] = np.bincount(p[n][seen], minlength=K)
        out[n, 2 * K:3 * K] = np.bincount(l[n][ok], minlength=K)
        P, G = p[n] != 0, l[n] != 0
        out[n, 3 * K:] = [(P & G).sum(), (P | G).sum(), (~P & ~G).sum(), G.sum()]
    return out


def run_reference(x, labels):
    """The reference's three functions on frames x [N, K, H, W], labels [N, H, W]."""
    xt, lt = torch.from_numpy(x.copy()), torch.from_numpy(labels.copy())
    ious, fscores, cls_count, vid = AM.calc_color_miou_fscore(xt, lt, T=T)
    ious2, cls2 = AM.calc_color_miou(xt, lt, T=T)
    binary = AM.calc_binary_miou(xt, lt)
    assert torch.equal(torch.from_numpy(x), xt) and torch.equal(torch.from_numpy(labels), lt)
    vid = np.array([float(v) for v in vid], dtype=np.float32)
    for v in list(vid[np.isfinite(vid)]) + [float(binary)]:
        assert v >= MARGIN, v
    return dict(ious=ious.numpy(), fscores=fscores.numpy(), cls_count=cls_count.numpy(), vid=vid, ious2=ious2.numpy(),
                cls2=cls2.numpy(), binary=np.array(binary.numpy(), dtype=np.float32))


def case(out, name, rs, K, hw):
    x, labels, amax = draw(rs, K, hw)
    assert (amax != K - 1).all() and (amax[0, 1] == 0).all() and (amax[1, 2] != 0).any()
    H, W = hw
    flat_x, flat_l = x.reshape(B * T, K, H, W), labels.reshape(B * T, H, W)
    out[f"{name}_logits"], out[f"{name}_labels"] = x, labels
    out[f"{name}_counts"] = counts_f64(amax, labels, K)
    runs = {"one": run_reference(flat_x, flat_l), "a": run_reference(x[0], labels[0]), "b": run_reference(x[1], labels[1])}
    for run, r in runs.items():
        for key, v in r.items():
            out[f"{name}_{run}_{key}"] = v
    # the two calls added as the driver adds them; in exact arithmetic they equal the one call
    for key in ("ious", "fscores", "cls_count"):
        out[f"{name}_two_{key}"] = runs["a"][key] + runs["b"][key]
        np.testing.assert_allclose(out[f"{name}_two_{key}"], runs["one"][key], rtol=1e-6, atol=0)


def build():
    out = {}
    case(out, "vec", np.random.RandomState(71), 5, (24, 28))
    case(out, "sca", np.random.RandomState(72), 3, (7, 9))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--check", action="store_true", help="compare with the stored fixture instead of writing it")
    a = ap.parse_args()
    torch.manual_seed(0)
    out = build()
    path = os.path.join(a.out, "semval.npz")
    if a.check:
        z = np.load(path)
        assert sorted(z.files) == sorted(out)
        worst = max(float(np.nanmax(np.abs(z[k].astype(np.float64) - out[k].astype(np.float64)))) if out[k].size else 0.0 for k in out)
        assert all(np.array_equal(np.isnan(z[k]), np.isnan(out[k])) for k in out if out[k].dtype.kind == "f")
        print("max difference from the stored fixture:", worst)
        return
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
