"""Host restatements of the reference's training augmentation (dataset/*/visual/visual_aug.py, VisualAugmentation.train_aug) with
the draws given: what cavp_amd/augment.py + csrc/augment.hip are tested against.

ref_pil(...) is the chain written with PIL calls only - the calls torchvision's PIL backend makes for the transforms the
reference uses.  The tests do not need torchvision: the mapping torchvision -> PIL below is taken from torchvision's published
source (transforms/_functional_pil.py) and has NOT been checked against a running torchvision:

    visual_aug.py:51-56  random_flip_h: F.hflip                      -> img.transpose(FLIP_LEFT_RIGHT)
    visual_aug.py:43-49  random_scales: w_, h_ = int(w_ * s), int(h_ * s); F.resize(image, (h_, w_), BICUBIC),
                         F.resize(label, (h_, w_), NEAREST)          -> img.resize((w_, h_), BICUBIC / NEAREST)
    visual_aug.py:13,61-62  ColorJitter(.5, .5, .5, .25): the four operations in the drawn order fn_idx,
                         0 adjust_brightness -> ImageEnhance.Brightness(img).enhance(b)
                         1 adjust_contrast   -> ImageEnhance.Contrast(img).enhance(c)
                         2 adjust_saturation -> ImageEnhance.Color(img).enhance(s)
                         3 adjust_hue        -> img.convert("HSV"), H += uint8(hue * 255) in numpy uint8, back to RGB
    visual_aug.py:29-35  random_crop_with_padding: w_, h_ = image_.size; if min(h_, w_) < min(image_size):
                         res_w_ = max(image_size[0] - w_, 0); res_h_ = max(image_size[1] - h_, 0)   (image_size = (H, W): the
                         reference mixes height and width here, reproduced literally)
                         F.pad(image_, [0, 0, res_w_, res_h_], fill)  -> ImageOps.expand(img, (0, 0, res_w_, res_h_), fill)
                         the frame's fill (mean * 255 as floats) is truncated to ints by torchvision for non-"F" images; the mask's is 255
    visual_aug.py:37-39  RandomCrop.get_params + F.crop              -> img.crop((left, top, left + W, top + H))
    visual_aug.py:64-66  ToTensor, Normalize                         -> u8 / 255, (x - mean) / std   (normalise() below)

ref_np(...) is the same chain in numpy integer (and, where PIL has them, float) arithmetic, rule by rule: the specification the
kernels implement.  tests/test_augment_host.py holds the two equal, stage by stage."""
import numpy as np

COCO_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)
AVS_SCALES = (0.5, 0.75, 1.0)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22


def default_pad_fill(mean=MEAN):
    return tuple(int(255 * m) for m in mean)


def scaled_size(h, w, scale):
    """visual_aug.py:46 (int() of a product that is exact for scales that are multiples of 1/64)."""
    return int(h * scale), int(w * scale)


def pad_amounts(h, w, crop):
    """(right, bottom) of visual_aug.py:31-33 for a scaled image h x w, literally (tgt_h against the width)."""
    H, W = crop
    if min(h, w) < min(H, W):
        return max(H - w, 0), max(W - h, 0)
    return 0, 0


def padded_size(h, w, crop):
    r, b = pad_amounts(h, w, crop)
    return h + b, w + r


def hue_shift_u8(hue):
    """torchvision's np.uint8(hue_factor * 255): truncation towards zero, then mod 256."""
    return int(hue * 255) % 256


def normalise(u8_hwc, mean=MEAN, std=STD):
    """ToTensor + Normalize in float32, CHW."""
    x = u8_hwc.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return (x - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]


# ------------------------------------------------------------------------------------------------------------------ numpy rules
def bicubic_filter(x):
    x = np.abs(np.asarray(x, np.float64))
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def bicubic_coeffs(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc: (xmin [out], n [out], k [out, ksize] int64 at 22 fractional bits)."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int64)
    num = np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        w = bicubic_filter((np.arange(n) + lo - center + 0.5) * ss)
        ww = 0.0
        for v in w:           # the same left-to-right double sum
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        k = w * float(1 << PRECISION_BITS)
        kk[xx, :n] = np.where(k < 0, (-0.5 + k).astype(np.int64), (0.5 + k).astype(np.int64))   # C's (int): towards zero
        xmin[xx], num[xx] = lo, n
    return xmin, num, kk


def _resample_axis0(img, out_size):
    """One pass of PIL's 8-bit resample along axis 0 of [n, m, 3] uint8."""
    xmin, num, kk = bicubic_coeffs(img.shape[0], out_size)
    src = img.astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for i in range(out_size):
        acc = np.tensordot(kk[i, :num[i]], src[xmin[i]:xmin[i] + num[i]], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic(img, size):
    """Image.resize((w, h), BICUBIC) of an RGB image: horizontal pass, rounded and clipped to uint8, then the vertical one; a
    pass whose size does not change is skipped, the same size is a copy."""
    oh, ow = size
    if ow != img.shape[1]:
        img = _resample_axis0(img.transpose(1, 0, 2), ow).transpose(1, 0, 2)
    if oh != img.shape[0]:
        img = _resample_axis0(img, oh)
    return np.ascontiguousarray(img)


def nearest_index(in_size, out_size):
    """Image.resize(NEAREST): an affine walk in double, xo = a / 2, then xo += a per output index with a = in / out; the
    source index is the truncation of the ACCUMULATED sum (not of (i + .5) * a: the two differ at ties)."""
    a = float(in_size) / out_size
    xo = a * 0.5
    idx = np.empty(out_size, np.int64)
    for i in range(out_size):
        idx[i] = int(xo)
        xo += a
    return np.minimum(idx, in_size - 1)


def resize_nearest(mask, size):
    return mask[nearest_index(mask.shape[0], size[0])][:, nearest_index(mask.shape[1], size[1])]


def luma(rgb):
    """PIL's RGB -> L."""
    c = rgb.astype(np.int64)
    return ((c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, factor):
    """Image.blend(deg, img, factor) on uint8 arrays: the factor is a C float; inside [0, 1] the float result is truncated,
    outside it is clamped to [0, 255] first."""
    f = np.float32(factor)
    if f == np.float32(0.0):
        return deg.astype(np.uint8).copy()
    if f == np.float32(1.0):
        return img.astype(np.uint8).copy()
    a = deg.astype(np.float32)
    t = a + f * (img.astype(np.float32) - a)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, t.astype(np.int32))).astype(np.uint8)


def contrast_mean(rgb):
    """ImageEnhance.Contrast: int(mean(L) + 0.5) over the whole image, as the exact integer floor((2 sum + n) / 2n)."""
    L = luma(rgb)
    return int((2 * int(L.sum(dtype=np.int64)) + L.size) // (2 * L.size))


def rgb_to_hsv(rgb):
    """PIL's rgb2hsv (Convert.c): float steps for s and the channel ratios, double for the hue."""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    mx = np.where(grey, 1, maxc).astype(np.float32)
    s = cr / mx
    rc = (maxc - r).astype(np.float32) / cr
    gc = (maxc - g).astype(np.float32) / cr
    bc = (maxc - b).astype(np.float32) / cr
    rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == maxc, (bc - gc).astype(np.float64), np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _c_round(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int32)


def hsv_to_rgb(hsv):
    """PIL's hsv2rgb (Convert.c)."""
    h, s, v = (hsv[..., i].astype(np.int32) for i in range(3))
    hf = h.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int32)
    f = (hf - i).astype(np.float32).astype(np.float64)
    fs = (s.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    vf = v.astype(np.float64)
    p = np.clip(_c_round(vf * (1.0 - fs)), 0, 255)
    q = np.clip(_c_round(vf * (1.0 - fs * f)), 0, 255)
    t = np.clip(_c_round(vf * (1.0 - fs * (1.0 - f))), 0, 255)
    sel = i % 6
    r = np.choose(sel, [v, q, p, p, t, v])
    g = np.choose(sel, [t, v, v, q, p, p])
    b = np.choose(sel, [p, p, t, v, v, q])
    grey = s == 0
    return np.stack([np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)], axis=-1).astype(np.uint8)


def hue_shift(rgb, shift):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = hsv[..., 0] + np.uint8(shift)
    return hsv_to_rgb(hsv)


def jitter_np(img, order, b, c, s, shift, stages=None):
    for k, op in enumerate(order):
        if op == 0:
            img = blend(np.zeros_like(img), img, b)
        elif op == 1:
            m = contrast_mean(img)
            if stages is not None:
                stages["contrast_mean"] = m
            img = blend(np.full_like(img, m), img, c)
        elif op == 2:
            img = blend(np.repeat(luma(img)[..., None], 3, axis=2), img, s)
        else:
            img = hue_shift(img, shift)
        if stages is not None:
            stages[f"jitter{k}"] = img
    return img


def ref_np(frame, mask, crop, flip, scale, top, left, jitter=None, pad_fill=None):
    """frame u8 [h, w, 3], mask u8 [h, w]; jitter = None or (order, b, c, s, hue_shift_u8).  Returns (image u8 [H, W, 3], label u8
    [H, W], stages) - stages: every intermediate by name, for the stage-by-stage comparison."""
    H, W = crop
    fill = default_pad_fill() if pad_fill is None else tuple(pad_fill)
    st = {}
    if flip:
        frame, mask = frame[:, ::-1], mask[:, ::-1]
    st["flip"], st["flip_mask"] = frame, mask
    size = scaled_size(frame.shape[0], frame.shape[1], scale)
    if size != frame.shape[:2]:
        frame, mask = resize_bicubic(frame, size), resize_nearest(mask, size)
    st["resize"], st["resize_mask"] = frame, mask
    if jitter is not None:
        frame = jitter_np(frame, *jitter, stages=st)
    r, b = pad_amounts(size[0], size[1], crop)
    if r or b or min(size) < min(crop):
        big = np.empty((size[0] + b, size[1] + r, 3), np.uint8)
        big[...] = np.asarray(fill, np.uint8)
        big[:size[0], :size[1]] = frame
        bigm = np.full((size[0] + b, size[1] + r), 255, np.uint8)
        bigm[:size[0], :size[1]] = mask
        frame, mask = big, bigm
    st["pad"], st["pad_mask"] = frame, mask
    if top < 0 or left < 0 or top + H > frame.shape[0] or left + W > frame.shape[1]:
        raise ValueError("the crop does not fit (torchvision's RandomCrop.get_params raises here)")
    frame, mask = frame[top:top + H, left:left + W], mask[top:top + H, left:left + W]
    st["crop"], st["crop_mask"] = frame, mask
    return np.ascontiguousarray(frame), np.ascontiguousarray(mask), st


# ------------------------------------------------------------------------------------------------------------------------ PIL
def ref_pil(frame, mask, crop, flip, scale, top, left, jitter=None, pad_fill=None):
    """The same signature and results as ref_np, every step a PIL call (module docstring)."""
    from PIL import Image, ImageEnhance, ImageOps
    H, W = crop
    fill = default_pad_fill() if pad_fill is None else tuple(int(v) for v in pad_fill)
    st = {}
    x, y = Image.fromarray(np.ascontiguousarray(frame), "RGB"), Image.fromarray(np.ascontiguousarray(mask), "L")
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
    w_, h_ = x.size
    if min(h_, w_) < min(H, W):
        res_w_, res_h_ = max(H - w_, 0), max(W - h_, 0)
        x = ImageOps.expand(x, border=(0, 0, res_w_, res_h_), fill=fill)
        y = ImageOps.expand(y, border=(0, 0, res_w_, res_h_), fill=255)
    st["pad"], st["pad_mask"] = np.asarray(x), np.asarray(y)
    if top < 0 or left < 0 or top + H > x.size[1] or left + W > x.size[0]:
        raise ValueError("the crop does not fit (torchvision's RandomCrop.get_params raises here)")
    x, y = x.crop((left, top, left + W, top + H)), y.crop((left, top, left + W, top + H))
    st["crop"], st["crop_mask"] = np.asarray(x), np.asarray(y)
    return np.array(x), np.array(y), st


# --------------------------------------------------------------------------------------------------- parameter table, replay
N_PARAMS = 16


def params_row(flip, scale_idx, top, left, order=(0, 1, 2, 3), b=1.0, c=1.0, s=1.0, shift=0):
    """One row of the [B, 16] int32 parameter table of cavp_amd.augment (PARAM_FIELDS)."""
    row = np.zeros(N_PARAMS, np.int32)
    row[0], row[1], row[9], row[10], row[11] = flip, scale_idx, shift, top, left
    row[2:6] = order
    row[6:9] = np.asarray([b, c, s], np.float32).view(np.int32)
    return row


def replay_row(ref, frame, mask, crop, row, scales=COCO_SCALES, jitter=False, pad_fill=None):
    """ref (ref_pil or ref_np) on one staged sample with the draws of a table row."""
    jit = None
    if jitter:
        b, c, s = (float(v) for v in row[6:9].view(np.float32))
        jit = (tuple(int(v) for v in row[2:6]), b, c, s, int(row[9]))
    return ref(frame, mask, crop, int(row[0]), scales[int(row[1])], int(row[10]), int(row[11]), jit, pad_fill)
