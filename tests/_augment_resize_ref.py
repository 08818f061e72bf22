"""The reference's resize_flag = True augmentation (dataset/avss/visual/visual_aug.py: flip, random scale, ColorJitter, then a
RESIZE to the output size in place of pad + crop; test_aug resizes too), twice: `ref_pil_resize` - every step a PIL call, the
specification - and `ref_np_resize` - the same in integer numpy from the primitives of tests/_augment_ref.py, stage by stage.
`composed_nearest` is the one-table form of the mask's NEAREST of NEAREST that the device's plan kernel builds."""
import numpy as np

from tests import _augment_ref as R

MAX_RATIO = 8          # in / out of the second resize, per axis: what cavp_amd.augment.FrameAugment(resize=True) accepts


def ref_np_resize(frame, mask, out_size, flip, scale, jitter=None):
    """frame u8 [h, w, 3], mask u8 [h, w]; scale None = the test-time path (no flip, no scale, no jitter); jitter = None or (order,
    b, c, s, hue_shift_u8).  Returns (image u8 [H, W, 3], label u8 [H, W], stages)."""
    st = {}
    if scale is not None:
        if flip:
            frame, mask = frame[:, ::-1], mask[:, ::-1]
        st["flip"], st["flip_mask"] = frame, mask
        size = R.scaled_size(frame.shape[0], frame.shape[1], scale)
        frame, mask = R.resize_bicubic(frame, size), R.resize_nearest(mask, size)
        st["resize"], st["resize_mask"] = frame, mask
        if jitter is not None:
            frame = R.jitter_np(frame, *jitter, stages=st)
    frame, mask = R.resize_bicubic(frame, out_size), R.resize_nearest(mask, out_size)
    st["out"], st["out_mask"] = frame, mask
    return np.ascontiguousarray(frame), np.ascontiguousarray(mask), st


def ref_pil_resize(frame, mask, out_size, flip, scale, jitter=None):
    """The same signature and results, every step a PIL call."""
    from PIL import Image, ImageEnhance
    H, W = out_size
    st = {}
    x, y = Image.fromarray(np.ascontiguousarray(frame), "RGB"), Image.fromarray(np.ascontiguousarray(mask), "L")
    if scale is not None:
        if flip:
            x, y = x.transpose(Image.FLIP_LEFT_RIGHT), y.transpose(Image.FLIP_LEFT_RIGHT)
        st["flip"], st["flip_mask"] = np.asarray(x), np.asarray(y)
        w_, h_ = x.size
        w_, h_ = int(w_ * scale), int(h_ * scale)
        x, y = x.resize((w_, h_), Image.BICUBIC), y.resize((w_, h_), Image.NEAREST)
        st["resize"], st["resize_mask"] = np.asarray(x), np.asarray(y)
        if jitter is not None:
            order, b, c, s, shift = jitter
            for k, op in enumerate(order):
                if op == 0:
                    x = ImageEnhance.Brightness(x).enhance(b)
                elif op == 1:
                    e = ImageEnhance.Contrast(x)
                    st["contrast_mean"] = int(np.asarray(e.degenerate)[0, 0, 0])
                    x = e.enhance(c)
                elif op == 2:
                    x = ImageEnhance.Color(x).enhance(s)
                else:
                    h, sat, v = x.convert("HSV").split()
                    np_h = np.array(h, dtype=np.uint8)
                    np_h += np.uint8(shift)
                    x = Image.merge("HSV", (Image.fromarray(np_h, "L"), sat, v)).convert("RGB")
                st[f"jitter{k}"] = np.asarray(x)
    x, y = x.resize((W, H), Image.BICUBIC), y.resize((W, H), Image.NEAREST)
    st["out"], st["out_mask"] = np.asarray(x), np.asarray(y)
    return np.array(x), np.array(y), st


def composed_nearest(in_size, scaled_size, out_size, mirror=False):
    """Source index of every output index through both NEAREST walks (scaled -> out, in -> scaled), the first consumed while the
    second advances: both are monotone, so no table of the scaled size is needed."""
    a1, a2 = float(in_size) / scaled_size, float(scaled_size) / out_size
    x1, x2, at = a1 * 0.5, a2 * 0.5, 0
    tab = np.empty(out_size, np.int64)
    for i in range(out_size):
        s1 = min(int(x2), scaled_size - 1)
        while at < s1:
            x1 += a1
            at += 1
        s = min(int(x1), in_size - 1)
        tab[i] = in_size - 1 - s if mirror else s
        x2 += a2
    return tab


def replay_row(ref, frame, mask, out_size, row, scales=R.AVS_SCALES, jitter=False, identity=False):
    """ref (ref_pil_resize or ref_np_resize) on one staged sample with the draws of a parameter-table row (words 10, 11 unused)."""
    if identity:
        return ref(frame, mask, out_size, 0, None)
    jit = None
    if jitter:
        b, c, s = (float(v) for v in row[6:9].view(np.float32))
        jit = (tuple(int(v) for v in row[2:6]), b, c, s, int(row[9]))
    return ref(frame, mask, out_size, int(row[0]), scales[int(row[1])], jit)


def ratios_ok(h, w, out_size, scale):
    """Every condition the device variant sets, on the reference's own sizes: a non-empty scaled image and in / out <= 8."""
    sh, sw = R.scaled_size(h, w, scale) if scale is not None else (h, w)
    return sh >= 1 and sw >= 1 and sh <= MAX_RATIO * out_size[0] and sw <= MAX_RATIO * out_size[1]
