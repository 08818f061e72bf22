"""Writes tests/golden/augment.npz: the inputs, the draws and what tests/_augment_ref.ref_pil (the reference's train_aug as PIL
calls) gives for the cases of tests/test_gpu_augment.py, with PIL.__version__.  Arrays and settings only.

    python tools/make_golden_augment.py

Stage 48 x 64; samples (29, 37) - a width not divisible by 4 -, (40, 56) - 4/3 ties -, (48, 64) - a full slot -, (13, 60) - one
side below the crop.  geo: crop 16 x 24, no jitter, every scale of the COCO list (the AVS list is its first three), flip off
and on, the crop origin cycling through 0, the maximum and an interior value; pad: crop 32 x 32 on the small samples at 0.5 and
1.0; bad: samples that cannot hold the crop under the reference's literal pad rule; jit: 24 samples, one per operation order."""
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _augment_ref as R  # noqa: E402

STAGE = (48, 64)
SIZES = [(29, 37), (40, 56), (48, 64), (13, 60)]
GEO_CROP, PAD_CROP, JIT_CROP = (16, 24), (32, 32), (32, 32)


def origin(kind, room):
    return (0, room, room // 2 if room > 1 else room)[kind]


def main():
    import PIL
    rng = np.random.default_rng(20240611)
    frames = rng.integers(0, 256, (len(SIZES),) + STAGE + (3,), dtype=np.uint8)
    masks = rng.choice(np.array([0, 1, 2, 3, 7, 255], np.uint8), (len(SIZES),) + STAGE)
    for i in range(len(SIZES)):     # smooth regions too: random bytes alone rarely sit on a rounding boundary of the jitter
        h, w = SIZES[i]
        yy, xx = np.mgrid[0:h // 2, 0:w // 2]
        frames[i, :h // 2, :w // 2] = np.stack([(5 * yy + 3 * xx) % 256, (250 - 7 * xx) % 256, (11 * yy) % 256], -1)
    out = {"frames": frames, "masks": masks, "sizes": np.asarray(SIZES, np.int32), "stage": np.asarray(STAGE, np.int32),
           "scales": np.asarray(R.COCO_SCALES), "mean": np.asarray(R.MEAN), "std": np.asarray(R.STD),
           "pad_fill": np.asarray(R.default_pad_fill(), np.int32), "pil_version": np.asarray(PIL.__version__),
           "geo_crop": np.asarray(GEO_CROP, np.int32), "pad_crop": np.asarray(PAD_CROP, np.int32),
           "jit_crop": np.asarray(JIT_CROP, np.int32)}

    def corner(i):
        h, w = SIZES[i]
        return frames[i, :h, :w], masks[i, :h, :w]

    def record(prefix, cases, crop, jitter=False):
        rows, imgs, lbls, means = [], [], [], []
        for i, row in cases:
            img, lbl, st = R.replay_row(R.ref_pil, *corner(i), crop, row, jitter=jitter)
            rows.append(row); imgs.append(img); lbls.append(lbl); means.append(st.get("contrast_mean", -1))
        out[prefix + "_sample"] = np.asarray([i for i, _ in cases], np.int32)
        out[prefix + "_params"] = np.stack(rows)
        out[prefix + "_image"] = np.stack(imgs)
        out[prefix + "_mask"] = np.stack(lbls)
        if jitter:
            out[prefix + "_mean"] = np.asarray(means, np.int32)

    geo, bad, n = [], [], 0
    for i, (h, w) in enumerate(SIZES):
        for si, s in enumerate(R.COCO_SCALES):
            ph, pw = R.padded_size(*R.scaled_size(h, w, s), GEO_CROP)
            for flip in (0, 1):
                if ph < GEO_CROP[0] or pw < GEO_CROP[1]:
                    if flip == 0:
                        bad.append((i, R.params_row(0, si, 0, 0)))
                    continue
                geo.append((i, R.params_row(flip, si, origin(n % 3, ph - GEO_CROP[0]), origin((n // 3 + n) % 3, pw - GEO_CROP[1]))))
                n += 1
    record("geo", geo, GEO_CROP)
    out["bad_sample"] = np.asarray([i for i, _ in bad], np.int32)
    out["bad_params"] = np.stack([r for _, r in bad])

    pad = []
    for i in (3, 0):
        for si in (0, 2):
            ph, pw = R.padded_size(*R.scaled_size(*SIZES[i], R.COCO_SCALES[si]), PAD_CROP)
            pad.append((i, R.params_row(0, si, (ph - PAD_CROP[0]) // 2, (pw - PAD_CROP[1]) // 2)))
    record("pad", pad, PAD_CROP)

    # jitter: sample 1 (40 x 56) at 1.25 -> 50 x 70; factors include the clamping ends; hue 231 is a negative draw after the wrap
    facs = [(1.5, 0.5, 1.5), (0.5, 1.5, 0.5), (float(np.float32(0.8123)), float(np.float32(1.2071)), float(np.float32(0.6337)))]
    jit = []
    for k, order in enumerate(itertools.permutations(range(4))):
        b, c, s = facs[k % 3]
        jit.append((1, R.params_row(k % 2, 3, (k * 5) % 19, (k * 7) % 39, order, b, c, s, (0, 63, 231)[(k // 3 + k) % 3])))
    record("jit", jit, JIT_CROP, jitter=True)
    path = os.path.join(REPO, "tests", "golden", "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(geo), "geo,", len(bad), "bad,", len(pad), "pad,", len(jit), "jit cases")


if __name__ == "__main__":
    main()
