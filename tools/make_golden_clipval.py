#!/usr/bin/env python3
"""Generate tests/golden/clip_validation.npz by running the REFERENCE metric classes (read-only import of utils/eval_utils.py from
/root/reference) through the validation loop of trainer/trainer_cavp_avss_image.py:295-349, restated here (the trainer module
itself cannot be imported), on the CPU.

Authoring-container only, on the recipe of tools/make_golden_metrics.py: the stub packages of tools/_shims and Tensor.cuda patched
to the identity.

Two cases, 16 x 20 frames (320 pixels, so that the reference's `count > 100` threshold is in reach), logits stored int8-quantised
(value / 8 on use):
  a_*  K = C = 8, 3 clips x 5 frames, mask_num = (5, 0, 3).  The labels hold frames with exactly 3 and exactly 2 qualifying values,
       a value at exactly 100 and one at 101 pixels, a frame whose third qualifying value is 255, a frame where K and K + 1 have 57
       pixels each (neither qualifies), and a frame where -1 and 255 together make the third value; the clip with mask_num = 0 and
       the tail of the third clip hold multi-source frames that must not be read.
  b_*  K = C = 71, 1 clip x 3 frames, mask_num = 3.
Stored per case: logits_q, labels, mask_num, results (the reference's ten rounded numbers: ALL then MS), M (both integer matrices
[2, K+1, K] as the numpy restatement below computes them; their first K rows equal the reference's confusion matrices, checked
here) and frames (frames fed to the ALL / the MS accumulators).

usage: python tools/make_golden_clipval.py [--out tests/golden]
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
import utils.eval_utils as EU  # noqa: E402

H, W = 16, 20


def frame(rs, spec):
    """A label frame from {value: pixel count}, the pixels in random order."""
    flat = np.concatenate([np.full(n, v, dtype=np.int64) for v, n in spec.items()])
    assert flat.size == H * W, flat.size
    return rs.permutation(flat).reshape(H, W)


def logits_for(rs, labels, C):
    """int8 logits in [-4, 4] (many exact ties); ~60 % of the pixels with a label < C get that class as a clear maximum."""
    q = rs.randint(-4, 5, size=labels.shape[:2] + (C,) + labels.shape[2:]).astype(np.int8)
    hit = (labels >= 0) & (labels < C) & (rs.rand(*labels.shape) < 0.6)
    b, t, y, x = np.nonzero(hit)
    q[b, t, labels[hit], y, x] = 5
    return q


def confusion(logits, label, K, ignore):
    """Integer restatement: M[(K+1) x K], row t < K or K for t >= K; pixels with t >= 0 and t != ignore."""
    p = torch.from_numpy(logits).argmax(1).numpy().ravel()
    t = label.ravel()
    ok = (t >= 0) & (t != ignore)
    row = np.where(t[ok] < K, t[ok], K)
    return np.bincount(row * K + p[ok], minlength=(K + 1) * K).reshape(K + 1, K).astype(np.int64)


def run_case(out, name, K, lq, labels, mask_num):
    """The reference loop: one clip per batch, one frame per forward; `logits` stands in for the model's avl_map_logits."""
    miou, miou_ms = (EU.MIoU(num_classes=K, ignore_index=255, local_rank=0) for _ in range(2))
    fg, fg_ms = (EU.ForegroundDetect(num_classes=K, local_rank=0) for _ in range(2))
    M = np.zeros((2, K + 1, K), dtype=np.int64)
    frames = [0, 0]
    for b in range(labels.shape[0]):
        pix_label = torch.from_numpy(labels[b].copy())          # the reference's MIoU writes -1 into it
        for i in range(int(mask_num[b])):
            avl_map_logits = torch.from_numpy(lq[b, i, None].astype(np.float32) / 8)
            curr_pix_label = pix_label[i]
            m = confusion(avl_map_logits.numpy(), labels[b, i], K, 255)
            fg(avl_map_logits, curr_pix_label)
            miou(avl_map_logits, curr_pix_label)
            M[0] += m
            frames[0] += 1
            uniq_id, count = curr_pix_label.unique(return_counts=True)
            valid_id = uniq_id[count > 100]
            if valid_id.shape[0] > 2:
                fg_ms(avl_map_logits, curr_pix_label)
                miou_ms(avl_map_logits, curr_pix_label)
                M[1] += m
                frames[1] += 1
    for k, f in enumerate((fg, fg_ms)):
        assert np.array_equal(np.asarray(f.confusion_matrix_), M[k, :K].astype(np.float64)), "restatement != reference"
    res = [float(v) for v in EU.get_performance(miou, fg)] + [float(v) for v in EU.get_performance(miou_ms, fg_ms)]
    out[f"{name}_logits_q"] = lq
    out[f"{name}_labels"] = labels
    out[f"{name}_mask_num"] = np.asarray(mask_num, dtype=np.int64)
    out[f"{name}_results"] = np.array(res, dtype=np.float64)
    out[f"{name}_M"] = M
    out[f"{name}_frames"] = np.array(frames, dtype=np.int64)
    print(name, "frames", frames, "results", res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    rs = np.random.RandomState(4321)
    out = {}

    K = 8
    three = {0: 110, 1: 105, 2: 105}                    # exactly 3 qualifying values: multi-source
    two = {0: 160, 3: 160}                              # exactly 2
    edge = {0: 119, 4: 100, 5: 101}                     # 100 pixels do not qualify, 101 do: 2 values
    third_255 = {0: 110, 6: 105, 255: 105}              # the ignore value is the third one: multi-source
    large = {0: 105, 7: 101, K: 57, K + 1: 57}          # K and K + 1 are values of their own: 2 values
    neg = {0: 110, 2: 105, 255: 55, -1: 50}             # -1 and 255 are one value of 105 pixels: multi-source
    clips = [[three, two, edge, third_255, large],      # mask_num = T
             [three, third_255, neg, three, three],     # mask_num = 0: never read
             [neg, large, three, three, third_255]]     # mask_num = 3: the last two are not read
    labels = np.stack([np.stack([frame(rs, s) for s in clip]) for clip in clips])
    run_case(out, "a", K, logits_for(rs, labels, K), labels, [5, 0, 3])

    K = 71
    spread = rs.randint(0, K, size=H * W).astype(np.int64)       # ~4.5 pixels per class: no value qualifies
    labels = np.stack([np.stack([frame(rs, {0: 110, 5: 105, 70: 105}), frame(rs, {0: 200, 33: 120}), spread.reshape(H, W)])])
    run_case(out, "b", K, logits_for(rs, labels, K), labels, [3])

    path = os.path.join(a.out, "clip_validation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
