"""The pictures of the reference's image upload on the GPU: what Tensorboard.upload_wandb_image (utils/tensor_board.py:90-139) makes
on the host from four whole-tensor .cpu() copies - the de-normalised frame `x`, the colour-coded label `y` and the colour-coded
prediction `y_tilde` of every frame - as one launch of csrc/preview.hip (two with a resize) that reads the logits once and leaves
5 bytes per pixel to copy.  With the mask of model.predict / ops.seg_predict as the prediction source the full-resolution logits
are never made at all.

    pv = PreviewStage(num_classes=K, mean=(.485, .456, .406), std=(.229, .224, .225), ignore_index=255, size=None, device=dev)
    out = pv(image, labels, logits=logits)        # or mask=mask; image=None / labels=None drop their panel (show_x / show_y)
    out.x, out.y, out.y_tilde                     # device uint8 views [B, h, w, 3], [B, h, w], [B, h, w] into out.buffer [B, 5*h*w]
    pics = pv.read(out)                           # one copy into a pinned buffer + one event wait: {"x": [...], "y": [...], "y_tilde": [...]}
    pv.check()                                    # raises if the device-side bad counter is non-zero

Opt-in and additive: nothing that exists changes.  The call has no host synchronisation and no host value that depends on a device
value: capturable in a hipGraph behind the eval forward or seg_predict (after one warm-up call, which allocates).  Inputs are never
modified.  The rules (restated in tests/_preview_ref.py, the C interface in include/cavp_hip.h "preview stage"):

x        uint8 [B, h, w, 3] from the normalised float32 NCHW image: per channel v = t * f32(std); v = v + f32(mean); u = v * 255 - three
         separately rounded float32 operations (DeNormalize's t.mul_(s).add_(m), then ToPILImage's pic.mul(255).byte()), no fused
         multiply-add - and the byte is u truncated toward zero, mod 256, as torch's CPU cast does.  A non-finite u or |u| >= 2^31
         writes 0 and is counted as bad.
y        uint8 [B, h, w]: the label mod 256 (colorize_mask's mask.astype(numpy.uint8): -1 -> 255, 259 -> 3).
y_tilde  uint8 [B, h, w]: the prediction - torch.argmax of float32 NCHW logits (first maximal index, a NaN counts as the maximum), or
         the uint8 mask as it is - overwritten with 255 where the raw label equals ignore_index (compared before the wrap).  Without
         labels nothing is overwritten, as in generate_image.
palette  y and y_tilde are palette INDICES; pv.palette is the 768-entry list that colorize_mask(get_pallete(num_classes)) leaves
         behind (entries beyond K are 0, the last entry is white), applied on the host by read().
size     optional (h, w): all three panels through Image.resize(NEAREST), the reference's resize=True with (256, 256), as a byte
         gather through two index tables made once per input size on the host."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

MAX_BATCH, MAX_CLASSES = 1024, 256


def palette(num_classes: int) -> list:
    """The 768 palette bytes of the reference's pictures: class j takes bit 3k + c of j as bit 7 - k of channel c (the PASCAL VOC
    colour map) for j < num_classes, the literal black / white pair for num_classes == 2, zeros beyond, and white as entry 255."""
    k = int(num_classes)
    pal = [0] * 768
    if k == 2:
        pal[3:6] = [255, 255, 255]
    else:
        for j in range(k):
            for bit in range(8):
                for c in range(3):
                    pal[3 * j + c] |= ((j >> (3 * bit + c)) & 1) << (7 - bit)
    pal[765:768] = [255, 255, 255]
    return pal


def nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """Image.resize(NEAREST)'s source index of every output index: PIL walks xo = a / 2, xo += a in double with a = in / out and
    truncates the accumulated sum (tests/_augment_ref.nearest_index)."""
    a = float(in_size) / out_size
    xo = a * 0.5
    idx = np.empty(out_size, np.int32)
    for i in range(out_size):
        idx[i] = min(int(xo), in_size - 1)
        xo += a
    return idx


class PreviewResult:
    """Outputs of one PreviewStage call: device uint8 views x [B, h, w, 3], y [B, h, w], y_tilde [B, h, w] (x / y None when their
    panel is dropped) into the contiguous arena `buffer` [B, planes * h * w]: per image x, then y, then y_tilde."""
    __slots__ = ("buffer", "x", "y", "y_tilde", "hw", "source_hw", "_staging")

    def __init__(self, B, source_hw, hw, has_x, has_y, dev):
        planes = (3 if has_x else 0) + (1 if has_y else 0) + 1
        self.source_hw, self.hw = tuple(source_hw), tuple(hw)
        n = hw[0] * hw[1]
        self.buffer = torch.empty((B, planes * n), dtype=torch.uint8, device=dev)
        # the panels at the input size, gathered into `buffer` by the resize launch
        self._staging = (torch.empty((B, planes * source_hw[0] * source_hw[1]), dtype=torch.uint8, device=dev)
                         if self.source_hw != self.hw else None)
        self._carve(has_x, has_y)

    def _carve(self, has_x, has_y):
        n, o = self.hw[0] * self.hw[1], 0
        self.x = self.y = None
        if has_x:
            self.x, o = self.buffer[:, :3 * n].unflatten(1, self.hw + (3,)), 3 * n
        if has_y:
            self.y, o = self.buffer[:, o:o + n].unflatten(1, self.hw), o + n
        self.y_tilde = self.buffer[:, o:o + n].unflatten(1, self.hw)


class PreviewStage:
    """See the module docstring.  Limits: B <= max_batch <= 1024, num_classes <= 256, logits with at most 256 channels.  Inputs are
    contiguous device tensors and are never modified."""

    def __init__(self, num_classes: int, mean, std, ignore_index: int = 255, size=None, device=None, max_batch: int = 64):
        E = _lib.CavpError
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise E(f"PreviewStage: 1 <= num_classes <= {MAX_CLASSES}")
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise E(f"PreviewStage: 1 <= max_batch <= {MAX_BATCH}")
        ms = [np.asarray(v, dtype=np.float64).ravel() for v in (mean, std)]
        if ms[0].size != 3 or ms[1].size != 3 or not np.isfinite(np.concatenate(ms)).all():
            raise E("PreviewStage: mean and std are three finite numbers each (R, G, B)")
        if size is not None:
            size = tuple(int(v) for v in size)
            if len(size) != 2 or min(size) < 1:
                raise E("PreviewStage: size is (h, w) with h, w >= 1")
        self.K, self.ignore_index, self.size, self.max_batch = int(num_classes), int(ignore_index), size, int(max_batch)
        self.mean_std_host = np.concatenate(ms).astype(np.float32)      # f32(mean), f32(std): the scalars of mul_ / add_
        self.palette = palette(self.K)
        self._device = device
        self._state = None       # device buffers, allocated by the first call (the constructor touches no device)
        self._tables = {}        # (H, W) -> (row_tab, col_tab) on the device
        self._pinned = None

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("PreviewStage lives on a HIP device (there is no CPU fallback)")
            self.device = dev
            self._mean_std = torch.from_numpy(self.mean_std_host).to(dev)
            self._state = torch.zeros(4, dtype=torch.int64, device=dev)       # {bad_pixels, reserved x 3}
        return self._state

    def _resize_tables(self, hw):
        if hw not in self._tables:
            self._tables[hw] = tuple(torch.from_numpy(nearest_table(i, o)).to(self.device) for i, o in zip(hw, self.size))
        return self._tables[hw]

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, an image value had no byte (a non-finite value, or one of
        magnitude 2^31 or more after the scaling: it was written as 0)."""
        if self._state is None:
            raise _lib.CavpError("check: no PreviewStage call yet")
        bad = int(self._state[0].item())
        if bad:
            self._state[0:1].zero_()
            raise _lib.CavpError(f"PreviewStage: {bad} image value(s) non-finite or beyond 2^31 after de-normalisation (written as 0)")

    # ---- the call -----------------------------------------------------------------------------------------------------------
    def _check_inputs(self, image, labels, logits, mask):
        E = _lib.CavpError
        if (logits is None) == (mask is None):
            raise E("PreviewStage: give exactly one of logits= and mask=")
        if logits is not None:
            if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 4:
                raise E("PreviewStage: logits must be float32 [B, C, H, W]")
            if not 1 <= logits.shape[1] <= 256:
                raise E(f"PreviewStage: a palette index holds at most 256 classes, the logits have {logits.shape[1]} channels")
            pred, B, hw = logits, logits.shape[0], tuple(logits.shape[2:])
        else:
            if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() != 3:
                raise E("PreviewStage: mask must be uint8 [B, H, W]")
            pred, B, hw = mask, mask.shape[0], tuple(mask.shape[1:])
        if not 1 <= B <= self.max_batch:
            raise E(f"PreviewStage: batch {B} outside [1, max_batch = {self.max_batch}]")
        if hw[0] < 1 or hw[1] < 1:
            raise E("PreviewStage: empty images are not supported")
        if image is not None and (not isinstance(image, torch.Tensor) or image.dtype != torch.float32
                                  or tuple(image.shape) != (B, 3) + hw):
            raise E(f"PreviewStage: image must be float32 {(B, 3) + hw}")
        if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int64, torch.uint8)
                                   or tuple(labels.shape) not in ((B,) + hw, (B, 1) + hw)):
            raise E(f"PreviewStage: labels must be int64 or uint8 {(B,) + hw} or {(B, 1) + hw}")
        for name, t in (("image", image), ("labels", labels), ("logits", logits), ("mask", mask)):
            if t is not None and not t.is_contiguous():
                raise E(f"PreviewStage: {name} must be contiguous")
        for name, t in (("image", image), ("labels", labels), ("logits", logits), ("mask", mask)):
            if t is not None and not t.is_cuda:
                raise E(f"PreviewStage: {name} is a CPU tensor; the preview stage needs HIP device tensors (no CPU fallback)")
        return pred, B, hw

    def __call__(self, image: Optional[torch.Tensor], labels: Optional[torch.Tensor], *, logits: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, out: Optional[PreviewResult] = None) -> PreviewResult:
        """out: a previous result of the same shapes and panels whose buffers are written again (static addresses for a captured
        graph)."""
        pred, B, hw = self._check_inputs(image, labels, logits, mask)
        state = self._ensure()
        dev = self.device
        for name, t in (("image", image), ("labels", labels), ("logits", logits), ("mask", mask)):
            if t is not None and t.device != dev:
                raise _lib.CavpError(f"PreviewStage lives on {dev}, {name} on {t.device}")
        has_x, has_y = image is not None, labels is not None
        out_hw = self.size if self.size is not None else hw
        planes = (3 if has_x else 0) + (1 if has_y else 0) + 1
        if out is None:
            out = PreviewResult(B, hw, out_hw, has_x, has_y, dev)
        elif (not isinstance(out, PreviewResult) or out.source_hw != hw or out.hw != out_hw or (out.x is not None) != has_x
              or (out.y is not None) != has_y or tuple(out.buffer.shape) != (B, planes * out_hw[0] * out_hw[1])
              or out.buffer.device != dev or out.buffer.dtype != torch.uint8 or not out.buffer.is_contiguous()):
            raise _lib.CavpError("PreviewStage: out= was made for other shapes or panels")
        lib = _lib.load()
        st = C.c_void_p(_stream())
        HW = hw[0] * hw[1]
        arena = out._staging if out._staging is not None else out.buffer
        base = arena.data_ptr()
        x_ptr = C.c_void_p(base) if has_x else None
        y_ptr = C.c_void_p(base + (3 * HW if has_x else 0)) if has_y else None
        yt_ptr = C.c_void_p(base + (planes - 1) * HW)
        _lib.check(lib.cavp_preview_panels(_ptr(image), _ptr(self._mean_std) if has_x else None, _ptr(labels),
                                           1 if has_y and labels.dtype == torch.uint8 else 0, _ptr(pred), 1 if mask is not None else 0, B,
                                           logits.shape[1] if logits is not None else 0, HW, self.ignore_index, x_ptr, y_ptr, yt_ptr,
                                           planes * HW, _ptr(state), st), "cavp_preview_panels")
        if out._staging is not None:
            rows, cols = self._resize_tables(hw)
            _lib.check(lib.cavp_preview_resize(_ptr(arena), _ptr(out.buffer), _ptr(rows), _ptr(cols), B, hw[0], hw[1], out_hw[0], out_hw[1],
                                               1 if has_x else 0, 1 if has_y else 0, st), "cavp_preview_resize")
        return out

    # ---- the host side ------------------------------------------------------------------------------------------------------
    def read(self, out: PreviewResult) -> dict:
        """The pictures of `out` on the host: ONE device-to-host copy of the arena (5 bytes per pixel with all panels) into a pinned
        buffer kept by the stage, one event wait.  {"x": [PIL RGB], "y": [PIL P], "y_tilde": [PIL P]} - the objects the reference
        hands to wandb.Image, the P images carrying pv.palette; a dropped panel has no key.  Without PIL the values are the numpy
        arrays (x [h, w, 3], y and y_tilde [h, w] palette indices)."""
        n = out.buffer.numel()
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        host = self._pinned[:n]
        host.copy_(out.buffer.view(-1), non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        B = out.buffer.shape[0]
        arena = host.numpy().reshape(B, -1).copy()       # the pinned buffer is written again by the next read
        h, w = out.hw
        hw, o, panels = h * w, 0, {}
        if out.x is not None:
            panels["x"], o = [arena[b, :3 * hw].reshape(h, w, 3) for b in range(B)], 3 * hw
        if out.y is not None:
            panels["y"], o = [arena[b, o:o + hw].reshape(h, w) for b in range(B)], o + hw
        panels["y_tilde"] = [arena[b, o:o + hw].reshape(h, w) for b in range(B)]
        try:
            from PIL import Image
        except ImportError:
            return panels
        return {k: [self._picture(Image, k, a) for a in v] for k, v in panels.items()}

    def _picture(self, Image, panel, a):
        if panel == "x":
            return Image.fromarray(a)
        pic = Image.fromarray(a).convert("P")
        pic.putpalette(self.palette)
        return pic
