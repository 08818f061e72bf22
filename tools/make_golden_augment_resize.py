"""Writes tests/golden/augment_resize.npz: the inputs, the draws and what tests/_augment_resize_ref.ref_pil_resize (the reference's
resize_flag = True train_aug / test_aug as PIL calls) gives for the cases of tests/test_gpu_augment_resize.py, with
PIL.__version__.  Arrays and settings only.

    python tools/make_golden_augment_resize.py

Frame sets (each with its staging slot): main - stage 192 x 64, frames (192, 64), (150, 61), (37, 29), output 24 x 72: vertical
ratio 8 at scale 1 (33+ taps), a horizontal upscale, two tile rows, a ragged second tile column, an odd width; coco - stage
96 x 64 under the COCO scale list at 1.25 and 2.0 (2 * 96 = 8 * 24); ident - (48, 64) at scale 1 to 48 x 64, an exact copy;
chain - 16 -> 12 -> 9, the NEAREST of NEAREST ties.  Case groups: geo (main: every AVS scale x flip off / on), jit (main, sample
1 at 0.75: one case per operation order), eval (main: the test-time path), coco, ident, chain.

Every case is checked here to stay inside the device variant's conditions on the reference's own sizes (a non-empty scaled
image, every in / out ratio <= 8) and ref_np_resize is checked against ref_pil_resize."""
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _augment_ref as R  # noqa: E402
from tests import _augment_resize_ref as RR  # noqa: E402

SETS = {   # name: (stage, sizes, output, scale list)
    "main": ((192, 64), [(192, 64), (150, 61), (37, 29)], (24, 72), R.AVS_SCALES),
    "coco": ((96, 64), [(96, 64), (75, 61)], (24, 72), R.COCO_SCALES),
    "ident": ((48, 64), [(48, 64)], (48, 64), R.AVS_SCALES),
    "chain": ((16, 16), [(16, 16)], (9, 9), R.AVS_SCALES),
}
GROUPS = {"geo": "main", "jit": "main", "eval": "main", "coco": "coco", "ident": "ident", "chain": "chain"}


def make_set(rng, stage, sizes):
    """Smooth ramps with a band of random bytes: the ramps sit on the rounding boundaries of the jitter, the noise drives the
    bicubic overshoot into the clip; masks are blobs of a few classes with 255 borders."""
    n = len(sizes)
    yy, xx = np.mgrid[0:stage[0], 0:stage[1]]
    frames = np.empty((n,) + stage + (3,), np.uint8)
    masks = np.zeros((n,) + stage, np.uint8)
    for i, (h, w) in enumerate(sizes):
        frames[i] = np.stack([(5 * yy + 3 * xx + 40 * i) % 256, (250 - 7 * xx + yy) % 256, (11 * yy + i) % 256], -1)
        by, bx = yy // 12, xx // 9          # flat colour blocks on the left (they keep the fixture small), ramps on the right
        flat = np.stack([(37 * by + 91 * bx) % 256, (201 * by + 13 * bx + 7 * i) % 256, (59 * by + 150 * bx) % 256], -1).astype(np.uint8)
        frames[i, :, :w // 2] = flat[:, :w // 2]
        band = slice(h // 3, h // 3 + max(h // 8, 2))
        frames[i, band] = rng.integers(0, 256, frames[i, band].shape, dtype=np.uint8)
        masks[i] = ((yy // 5 + xx // 7 + i) % 4).astype(np.uint8) * ((yy * 3 + xx) % 11 > 2)
        masks[i, (yy + 2 * xx) % 23 == 0] = 255
    return frames, masks


def main():
    import PIL
    rng = np.random.default_rng(20240719)
    out = {"pil_version": np.asarray(PIL.__version__), "mean": np.asarray(R.MEAN), "std": np.asarray(R.STD)}
    data = {}
    for name, (stage, sizes, size_out, scales) in SETS.items():
        frames, masks = make_set(rng, stage, sizes)
        data[name] = (frames, masks, sizes, size_out, scales)
        out.update({f"{name}_frames": frames, f"{name}_masks": masks, f"{name}_sizes": np.asarray(sizes, np.int32),
                    f"{name}_stage": np.asarray(stage, np.int32), f"{name}_out": np.asarray(size_out, np.int32),
                    f"{name}_scales": np.asarray(scales)})

    def record(group, cases, jitter=False, identity=False):
        frames, masks, sizes, size_out, scales = data[GROUPS[group]]
        rows, imgs, lbls, means = [], [], [], []
        for i, row in cases:
            h, w = sizes[i]
            assert RR.ratios_ok(h, w, size_out, None if identity else scales[int(row[1])]), (group, i, row[:2])
            args = (frames[i, :h, :w], masks[i, :h, :w], size_out, row)
            img, lbl, st = RR.replay_row(RR.ref_pil_resize, *args, scales=scales, jitter=jitter, identity=identity)
            img_np, lbl_np, st_np = RR.replay_row(RR.ref_np_resize, *args, scales=scales, jitter=jitter, identity=identity)
            assert np.array_equal(img, img_np) and np.array_equal(lbl, lbl_np), (group, i)
            rows.append(row); imgs.append(img); lbls.append(lbl); means.append(st.get("contrast_mean", -1))
        out[group + "_sample"] = np.asarray([i for i, _ in cases], np.int32)
        out[group + "_params"] = np.stack(rows)
        out[group + "_image"] = np.stack(imgs)
        out[group + "_mask"] = np.stack(lbls)
        if jitter:
            out[group + "_mean"] = np.asarray(means, np.int32)
        return len(cases)

    counts = {}
    counts["geo"] = record("geo", [(i, R.params_row(flip, si, 0, 0)) for i in range(3) for si in range(3) for flip in (0, 1)])
    facs = [(1.5, 0.5, 1.5), (0.5, 1.5, 0.5), (float(np.float32(0.8123)), float(np.float32(1.2071)), float(np.float32(0.6337)))]
    jit = []
    for k, order in enumerate(itertools.permutations(range(4))):
        b, c, s = facs[k % 3]
        jit.append((1, R.params_row(k % 2, 1, 0, 0, order, b, c, s, (0, 63, 231)[(k // 3 + k) % 3])))
    counts["jit"] = record("jit", jit, jitter=True)
    counts["eval"] = record("eval", [(i, R.params_row(0, 0, 0, 0)) for i in range(3)], identity=True)
    counts["coco"] = record("coco", [(i, R.params_row((i + si) % 2, si, 0, 0)) for i in range(2) for si in (3, 6)])
    counts["ident"] = record("ident", [(0, R.params_row(0, 2, 0, 0))])
    assert np.array_equal(out["ident_image"][0], data["ident"][0][0])            # an exact copy
    counts["chain"] = record("chain", [(0, R.params_row(flip, 1, 0, 0)) for flip in (0, 1)])
    path = os.path.join(REPO, "tests", "golden", "augment_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ", ".join(f"{n} {g}" for g, n in counts.items()), "cases")


if __name__ == "__main__":
    main()
