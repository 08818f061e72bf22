"""Image labels from the pixel labels on the GPU: what the reference's data sets compute from the mask AFTER the transform, so that
FrameAugment's label can feed PairBuilder without a trip to the host - the VPO sets' COCO -> VPO class-index remap and class vector
(dataset/vpo_mono/multi_source/visual/visual_dataset.py:127-145), the AVSS sets' class vector and binary collapse
(dataset/avss/visual/visual_dataset.py:157-165), AVSBench's one_hot(mask.sum() != 0, 2) (dataset/avsbench_ms.py:135-136) - as two or
three launches of csrc/labels.hip with no host value that depends on a device value: capturable in a hipGraph between FrameAugment
and PairBuilder.

    st = LabelStage(num_classes=K, mode="multi_hot", remap=table, binary=False, ignore_index=255, device=dev, max_batch=Bmax)
    out = st(aug_out.label)             # contiguous device int64 or uint8 [B, H, W]; never modified
    out.img_label                       # int64 [B, K]: what PairBuilder takes
    out.label                           # int64 [B, H, W]: remapped / collapsed copy (the input itself if nothing changes it)
    st.check()                          # raises if the device-side bad counter is non-zero

Opt-in and additive: nothing that exists changes.  The rules, in the reference's order (restated in tests/_labels_ref.py, the C
interface in include/cavp_hip.h "label stage"):

remap (optional, int32 [256]): remap[v] is the new index of raw mask value v; -1 = "the reference would raise here" (its
class_dict / index_table lookup fails): such a pixel is counted as bad and keeps its value.  The reference's loop runs in place over
the value list taken before it - for each i of unique(label) other than 0 and 255, ascending, label[label == i] = remap[i] - so a pixel
moved to t > i is moved AGAIN at step t if t was in the raw image.  That is reproduced literally (per pixel in closed form, from a
presence mask of the raw image).

class vector: "multi_hot": img_label[b, c] = 1 iff some pixel of the (remapped) label equals c, c in [0, K); pixels equal to
ignore_index are left out, background 0 counts when present, an image of only 255 gives zeros.  A value outside [0, K) that is not
ignore_index makes one_hot raise in the reference; here it is counted as bad and ignored.  "any_foreground" (K = 2): [1, 0] if every
pixel is 0, else [0, 1] - a 255 pixel is non-zero, as in the reference's sum.

binary (optional): (label != ignore_index) & (label != 0) -> 1, applied after the class vector as in the AVSS data set.

Launches: presence(raw image; only with a remap) -> scan (remap + class bits + collapse + label copy) -> expand ([B, K] int64).
The per-image 256-bit masks are zero at rest and cleared again by the expand launch: nothing is memset outside the launches."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

MAX_BATCH, MAX_CLASSES = 1024, 256
MODES = ("multi_hot", "any_foreground")


class LabelResult:
    """Outputs of one LabelStage call, device tensors: img_label [B, K] i64; label [B, H, W] i64."""
    __slots__ = ("img_label", "label")

    def __init__(self, B, K, hw, dev, own_label: bool):
        self.img_label = torch.empty((B, K), dtype=torch.int64, device=dev)
        self.label = torch.empty((B,) + tuple(hw), dtype=torch.int64, device=dev) if own_label else None


class LabelStage:
    """See the module docstring.  Limits: B <= max_batch <= 1024, num_classes <= 256 (PairBuilder's limit), remap entries in
    [-1, 255], 0 <= ignore_index <= 255.  Inputs must be contiguous device tensors and are never modified."""

    def __init__(self, num_classes: int, mode: str = "multi_hot", remap=None, binary: bool = False, ignore_index: int = 255,
                 device=None, max_batch: int = 64):
        E = _lib.CavpError
        if mode not in MODES:
            raise E(f"LabelStage: mode is one of {MODES}")
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise E(f"LabelStage: 1 <= num_classes <= {MAX_CLASSES}")
        if mode == "any_foreground" and int(num_classes) != 2:
            raise E("LabelStage: any_foreground has num_classes = 2")
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise E(f"LabelStage: 1 <= max_batch <= {MAX_BATCH}")
        if not 0 <= int(ignore_index) <= 255:
            raise E("LabelStage: 0 <= ignore_index <= 255")
        self.K, self.mode, self.binary, self.ignore_index = int(num_classes), mode, bool(binary), int(ignore_index)
        self.max_batch = int(max_batch)
        self.remap_host = None
        if remap is not None:
            r = remap.detach().cpu().numpy() if isinstance(remap, torch.Tensor) else np.asarray(remap)
            if r.shape != (256,) or r.dtype.kind not in "iu":
                raise E("LabelStage: remap is an integer table of 256 entries (remap[v] = new index of raw value v, -1 = none)")
            if r.min() < -1 or r.max() > 255:
                raise E("LabelStage: remap entries lie in [-1, 255]")
            self.remap_host = np.ascontiguousarray(r.astype(np.int32))
        self._device = device
        self._state = None       # device buffers, allocated by the first call (the constructor touches no device)

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("LabelStage lives on a HIP device (there is no CPU fallback)")
            self.device = dev
            self._mask = torch.zeros((self.max_batch, 8), dtype=torch.int32, device=dev)     # zero at rest (see the docstring)
            self._raw_mask = torch.zeros((self.max_batch, 8), dtype=torch.int32, device=dev) if self.remap_host is not None else None
            self._remap = torch.from_numpy(self.remap_host).to(dev) if self.remap_host is not None else None
            self._state = torch.zeros(4, dtype=torch.int64, device=dev)       # {bad_pixels, reserved x 3}
        return self._state

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, a pixel had no remap entry or a value that is no class
        (where the reference's lookup or one_hot raises)."""
        if self._state is None:
            raise _lib.CavpError("check: no LabelStage call yet")
        bad = int(self._state[0].item())
        if bad:
            self._state[0:1].zero_()
            raise _lib.CavpError(f"LabelStage: {bad} pixel(s) without a remap entry or outside [0, {self.K}) and not {self.ignore_index}")

    @property
    def changes_label(self) -> bool:
        return self.remap_host is not None or self.binary

    # ---- the call -----------------------------------------------------------------------------------------------------------
    def _check_inputs(self, label):
        E = _lib.CavpError
        if not isinstance(label, torch.Tensor) or label.dtype not in (torch.int64, torch.uint8) or label.dim() != 3:
            raise E("LabelStage: label must be int64 or uint8 [B, H, W]")
        B = label.shape[0]
        if not 1 <= B <= self.max_batch:
            raise E(f"LabelStage: batch {B} outside [1, max_batch = {self.max_batch}]")
        if label.shape[1] < 1 or label.shape[2] < 1:
            raise E("LabelStage: empty images are not supported")
        if not label.is_cuda:
            raise E("LabelStage: label is a CPU tensor; the label stage needs HIP device tensors (no CPU fallback)")
        if not label.is_contiguous():
            raise E("LabelStage: label must be contiguous")
        return B

    def __call__(self, label: torch.Tensor, out: Optional[LabelResult] = None) -> LabelResult:
        """out: a previous result of the same shapes whose buffers are written again (static addresses for a captured graph)."""
        B = self._check_inputs(label)
        state = self._ensure()
        dev = self.device
        if label.device != dev:
            raise _lib.CavpError(f"LabelStage lives on {dev}, label on {label.device}")
        hw = tuple(label.shape[1:])
        own = self.changes_label or label.dtype != torch.int64
        if out is None:
            out = LabelResult(B, self.K, hw, dev, own)
        elif tuple(out.img_label.shape) != (B, self.K) or out.img_label.device != dev or (
                own and (out.label is None or out.label.shape != label.shape or out.label.data_ptr() == label.data_ptr())):
            raise _lib.CavpError("LabelStage: out= was made for other shapes")
        if not own:
            out.label = label
        lib = _lib.load()
        st = C.c_void_p(_stream())
        u8 = 1 if label.dtype == torch.uint8 else 0
        HW = hw[0] * hw[1]
        any_fg = 1 if self.mode == "any_foreground" else 0
        if self._remap is not None:
            _lib.check(lib.cavp_labels_presence(_ptr(label), u8, B, HW, _ptr(self._raw_mask), st), "cavp_labels_presence")
        _lib.check(lib.cavp_labels_scan(_ptr(label), u8, B, HW, self.K, any_fg, _ptr(self._remap), 1 if self.binary else 0,
                                        self.ignore_index, _ptr(self._raw_mask), _ptr(self._mask), _ptr(state),
                                        _ptr(out.label) if own else None, st), "cavp_labels_scan")
        _lib.check(lib.cavp_labels_expand(_ptr(self._mask), _ptr(self._raw_mask), B, self.K, any_fg, _ptr(out.img_label), st),
                   "cavp_labels_expand")
        return out
