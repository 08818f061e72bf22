"""Frame augmentation on the GPU: VisualAugmentation.train_aug of the reference (dataset/*/visual/visual_aug.py:58-67) - horizontal
flip, random rescale (BICUBIC frame, NEAREST mask), ColorJitter(.5, .5, .5, .25), pad to the crop size, random crop, ToTensor +
Normalize - on raw decoded uint8 frames and masks as three launches of csrc/augment.hip, with no host value that depends on a
device value: the call can be captured in a hipGraph as the `prologue` of CAVP.capture_train_step next to PairBuilder and
MelFrontEnd.  The host decodes, pads every sample into the top-left corner of a fixed staging slot, and copies once.

    aug = FrameAugment(crop=(H, W), mean=MEAN, std=STD, scales=COCO_SCALES, jitter=(.5, .5, .5, .25), seed=0, device=dev,
                       max_batch=Bmax, stage=(Hs, Ws))
    out = aug(frames, masks, sizes)        # frames u8 [B, Hs, Ws, 3] (HWC as decoded), masks u8 [B, Hs, Ws], sizes i32 [B, 2] = (h, w)
    out.image   # f32 [B, 3, H, W] normalised      out.label   # i64 [B, H, W]      out.params   # i32 [B, 16], see PARAM_FIELDS
    aug.eval_(frames, masks, sizes)        # test_aug: ToTensor + Normalize of the top-left H x W window

Opt-in and additive: nothing that exists changes.  The arithmetic is PIL's (the library torchvision's transforms call for PIL
images), restated rule by rule in tests/_augment_ref.py and DESIGN.md 4p, the C interface in include/cavp_hip.h ("frame
augmentation").

Randomness: without `params=` the plan kernel draws with Philox4x32-10 in the device sampler's convention from the
device state {seed, offset}; every call and every replay of a captured call advances the offset, `manual_seed()` resets it.  The
distributions are the reference's (flip = random() > 0.5; scale uniform over the list; the order of the four jitter operations
uniform over the 24 permutations; brightness, contrast, saturation U[0.5, 1.5]; hue U[-0.25, 0.25] turned into the uint8 added
to H as torchvision does, by truncating hue * 255 and wrapping mod 256; top uniform in [0, h' - H], left likewise) but the stream
is another one than Python's `random` and torch's generator: no seed reproduces the reference's values.  `params=` replaces the
draws - that is how the tests replay recorded ones.

Pad and crop follow the reference literally, including its height / width mix-up (visual_aug.py:31-33): with (h, w) the scaled
size, the pad triggers when min(h, w) < min(H, W), the right pad is max(H - w, 0) and the bottom pad max(W - h, 0).  For square
crops that is "pad to the crop".  Where torchvision would raise because the padded image cannot hold the crop, the sample is
counted in a device-side `bad` counter (as are staged sizes outside 1 <= h <= Hs, 1 <= w <= Ws and `params` fields out of range)
and rendered from clamped coordinates; nothing is read out of bounds; check() raises.

`resize=True` is the avss data set's `resize_flag=True` variant (visual_aug.py:31-35,71-72,81-82; main_avss_resize.py): flip, random
scale and jitter as above, then the image is RESIZED to `crop` (BICUBIC frame, NEAREST mask) instead of padded and cropped;
eval_() resizes too.  The same seed and offset give the same flip, scale and jitter draws (params[:, 0:10]) as the crop variant;
the crop origin is not drawn, top = left = 0, pad_fill is unused and no sample is "too small".  The frame goes through PIL's
sequence step by step - two-pass BICUBIC to the scaled size, the jitter chain on that uint8 image, a second two-pass BICUBIC to
H x W - so the scaled image is stored once in a scratch allocated with the device state: max_batch x floor(Hs * max(scales)) x
floor(Ws * max(scales)) x 4 bytes (52 MB at max_batch 32, stage 640 x 640, the AVS scales).  The second pass holds 34 taps:
stage_side * max(scales) <= 8 * crop_side on both axes (eval_: stage_side <= 8 * crop_side), the constructor raises otherwise;
`crop` may be larger than the stage (an upscale).  Launches: plan_resize -> contrast_mean (only with jitter) -> resize_store ->
resize_render; eval_: plan_resize -> resize_render on the staged frames.

Out of scope: decoding (stays on the host).  The data sets' class-index remap of the mask and their image labels are
cavp_amd/labels.py (LabelStage), which takes out.label.  The five copies of visual_aug.py were
compared: vpo_mono/single_source and vpo_stereo/single_source only add the "avs_sailent" setup name (= jitter=None, scales
(0.5, 0.75, 1.0)); vpo_stereo/multi_source additionally returns the flip decision, which is out.params[:, 0] here (the stereo
trainers swap the audio channels with it); avss adds the resize_flag branch (`resize=True`).  With resize_flag off all five compute
the same pixels."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from .ops import _ptr, _stream

MAX_BATCH, MAX_SCALES = 1024, 16
RESIZE_MAX_RATIO = 8        # in / out of the resize variant's second pass, per axis (34 taps)
COCO_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)
AVS_SCALES = (0.5, 0.75, 1.0)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# words of a row of the [B, 16] int32 parameter table (the three factors are float32 bit patterns: .view(torch.float32))
PARAM_FIELDS = ("flip", "scale", "order0", "order1", "order2", "order3", "brightness", "contrast", "saturation", "hue_shift", "top",
                "left", "scaled_h", "scaled_w", "contrast_mean", "bad")
N_PARAMS = len(PARAM_FIELDS)


class AugResult:
    """Outputs of one FrameAugment call, every field a device tensor: image [B, 3, H, W] f32, label [B, H, W] i64, params [B, 16]
    i32 (PARAM_FIELDS)."""
    __slots__ = ("image", "label", "params")

    def __init__(self, B, crop, dev):
        self.image = torch.empty((B, 3) + tuple(crop), dtype=torch.float32, device=dev)
        self.label = torch.empty((B,) + tuple(crop), dtype=torch.int64, device=dev)
        self.params = torch.empty((B, N_PARAMS), dtype=torch.int32, device=dev)

    def factors(self) -> torch.Tensor:
        """[B, 3] float32: the brightness, contrast and saturation factors of the table."""
        return self.params[:, 6:9].contiguous().view(torch.float32)


def make_params(flip, scale, top, left, order=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0, hue_shift=0) -> torch.Tensor:
    """One row of the parameter table (CPU int32 [16]) from plain values: stack rows and move them to the device for `params=`."""
    row = torch.zeros(N_PARAMS, dtype=torch.int32)
    row[0], row[1], row[9], row[10], row[11] = int(flip), int(scale), int(hue_shift), int(top), int(left)
    row[2:6] = torch.tensor([int(v) for v in order], dtype=torch.int32)
    row[6:9] = torch.tensor([brightness, contrast, saturation], dtype=torch.float32).view(torch.int32)
    return row


class FrameAugment:
    """See the module docstring.  Limits: B <= max_batch <= 1024; at most 16 scales, each a multiple of 1/64 in [0.5, 4] (both
    reference lists qualify; it makes the reference's int(w * s) an exact integer expression on the device and bounds the filter
    taps); crop <= stage (resize=True: any crop with stage_side * max(scales) <= 8 * crop_side).  Inputs must be contiguous device
    tensors and are never modified."""

    def __init__(self, crop, mean=IMAGENET_MEAN, std=IMAGENET_STD, scales=COCO_SCALES, jitter=(.5, .5, .5, .25), pad_fill=None,
                 seed: int = 0, device=None, max_batch: int = 64, stage=None, resize: bool = False):
        E = _lib.CavpError
        if stage is None or len(tuple(stage)) != 2 or len(tuple(crop)) != 2:
            raise E("FrameAugment: crop=(H, W) and stage=(Hs, Ws) are required")
        self.H, self.W = (int(v) for v in crop)
        self.Hs, self.Ws = (int(v) for v in stage)
        self.resize = bool(resize)
        if self.H < 1 or self.W < 1 or (not self.resize and (self.H > self.Hs or self.W > self.Ws)):
            raise E(f"FrameAugment: crop {(self.H, self.W)} must be positive and fit the stage {(self.Hs, self.Ws)}")
        if self.resize and (self.H > 16384 or self.W > 16384):
            raise E("FrameAugment: output sides above 16384 are not supported")
        if self.resize and pad_fill is not None:
            raise E("FrameAugment: resize=True has no pad: pad_fill must be left at its default")
        if self.Hs > 16384 or self.Ws > 16384:
            raise E("FrameAugment: stage sides above 16384 are not supported")
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise E(f"FrameAugment: 1 <= max_batch <= {MAX_BATCH}")
        self.max_batch = int(max_batch)
        scales = tuple(float(s) for s in scales)
        if not 1 <= len(scales) <= MAX_SCALES:
            raise E(f"FrameAugment: 1 to {MAX_SCALES} scales")
        for s in scales:
            if not math.isfinite(s) or s * 64 != int(s * 64):
                raise E(f"FrameAugment: scale {s} is not a multiple of 1/64 (n/64 keeps int(w * s) exact on the device)")
            if not 0.5 <= s <= 4.0:
                raise E(f"FrameAugment: scale {s} outside [0.5, 4]")
        self.scales = scales
        self._scales64 = (C.c_int32 * len(scales))(*[int(s * 64) for s in scales])
        # the resize variant's scaled image at its largest (floor(side * s) is exact: s is a multiple of 1/64)
        self._mh, self._mw = (self.Hs * max(self._scales64)) >> 6, (self.Ws * max(self._scales64)) >> 6
        if self.resize and (self._mh > RESIZE_MAX_RATIO * self.H or self._mw > RESIZE_MAX_RATIO * self.W):
            raise E(f"FrameAugment: resize=True reduces by at most {RESIZE_MAX_RATIO} per axis (34 filter taps): stage {(self.Hs, self.Ws)} "
                    f"x scale {max(scales)} = {(self._mh, self._mw)} exceeds {RESIZE_MAX_RATIO} x crop {(self.H, self.W)}")
        if len(mean) != 3 or len(std) != 3 or any(not float(s) > 0 for s in std):
            raise E("FrameAugment: mean and std have three entries, std > 0")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if jitter is not None and tuple(float(v) for v in jitter) != (.5, .5, .5, .25):
            raise E("FrameAugment: jitter is (.5, .5, .5, .25) - the reference's ColorJitter - or None")
        self.jitter = None if jitter is None else (.5, .5, .5, .25)
        # torchvision truncates a float fill for non-"F" images before it reaches PIL: int(255 * m)
        self.pad_fill = tuple(int(255 * m) for m in self.mean) if pad_fill is None else tuple(int(v) for v in pad_fill)
        if len(self.pad_fill) != 3 or any(not 0 <= v <= 255 for v in self.pad_fill):
            raise E("FrameAugment: pad_fill is three integers in 0..255")
        self._mean3, self._std3 = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        self._fill3 = (C.c_int32 * 3)(*self.pad_fill)
        self._device = device
        self._seed = int(seed)
        self._state = None       # device buffers, allocated by the first call (the constructor touches no device)
        self._last = None

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("FrameAugment lives on a HIP device (there is no CPU fallback)")
            self.device = dev
            self._state = torch.zeros(4, dtype=torch.int64, device=dev)       # {seed, offset, bad_inputs, reserved}
            self._near = torch.empty((self.max_batch, self.H + self.W), dtype=torch.int32, device=dev)
            self._lsum = torch.zeros(self.max_batch, dtype=torch.int64, device=dev)
            self._scratch = torch.empty((self.max_batch, self._mh, self._mw), dtype=torch.int32, device=dev) if self.resize else None
            self.manual_seed(self._seed)
        return self._state

    def manual_seed(self, seed: int) -> None:
        """Reset the seed and the call counter (offset 0).  A host-to-device write: not legal during a capture; graphs captured
        earlier see the new values on their next replay."""
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._seed = s - (1 << 64) if s >= (1 << 63) else s
        if self._state is not None:
            self._state[:2].copy_(torch.tensor([self._seed, 0], dtype=torch.int64))

    def rollback_ranges(self):
        """[(name, tensor, byte_offset, nbytes)]: {seed, offset} of the state block, the only state a call mutates (`bad_inputs`
        is a diagnostic and is not named).  For cavp_amd.rollback.StepRollback.add()."""
        return [("state", self._ensure(), 0, 16)]

    def offset(self) -> int:
        """Synchronises: the number of calls (and replays) since the last manual_seed()."""
        return int(self._ensure()[1].item())

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, a sample had a staged size outside the slot, an empty
        scaled image, a `params` field out of range, or could not hold the crop after the reference's pad rule (where
        torchvision's RandomCrop raises)."""
        if self._state is None:
            raise _lib.CavpError("check: no FrameAugment call yet")
        bad = int(self._state[2].item())
        if bad:
            self._state[2:3].zero_()
            raise _lib.CavpError(f"FrameAugment: {bad} sample(s) with a size outside the staging slot, a params field out of range "
                                 f"or a scaled image that cannot hold the crop (see out.params[:, 15])")

    # ---- the call -----------------------------------------------------------------------------------------------------------
    def _check_inputs(self, frames, masks, sizes, params):
        E = _lib.CavpError
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (self.Hs, self.Ws, 3):
            raise E(f"FrameAugment: frames must be uint8 [B, {self.Hs}, {self.Ws}, 3] (HWC)")
        B = frames.shape[0]
        if not 1 <= B <= self.max_batch:
            raise E(f"FrameAugment: batch {B} outside [1, max_batch = {self.max_batch}]")
        if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or tuple(masks.shape) != (B, self.Hs, self.Ws):
            raise E(f"FrameAugment: masks must be uint8 [B, {self.Hs}, {self.Ws}]")
        if not isinstance(sizes, torch.Tensor) or sizes.dtype != torch.int32 or tuple(sizes.shape) != (B, 2):
            raise E("FrameAugment: sizes must be int32 [B, 2] = (h, w)")
        if params is not None and (not isinstance(params, torch.Tensor) or params.dtype != torch.int32 or tuple(params.shape) != (B, N_PARAMS)):
            raise E(f"FrameAugment: params must be int32 [B, {N_PARAMS}]")
        for name, t in (("frames", frames), ("masks", masks), ("sizes", sizes), ("params", params)):
            if t is None:
                continue
            if not t.is_cuda:
                raise E(f"FrameAugment: {name} is a CPU tensor; the augmentation needs HIP device tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise E(f"FrameAugment: {name} must be contiguous")
        return B

    def _run(self, frames, masks, sizes, params, out, identity, launches=None):
        """launches: the subset to issue (tools/bench_augment.py times each alone, on the table the last plan left in `out`); None =
        all of ("plan", "mean", "render"), with "store" in front of "render" for resize=True."""
        if launches is None:
            launches = ("plan", "mean", "store", "render") if self.resize else ("plan", "mean", "render")
        B = self._check_inputs(frames, masks, sizes, params)
        state = self._ensure()
        dev = self.device
        if frames.device != dev or masks.device != dev or sizes.device != dev:
            raise _lib.CavpError(f"FrameAugment lives on {dev}, inputs on {frames.device}")
        if out is None:
            out = AugResult(B, (self.H, self.W), dev)
        elif tuple(out.image.shape) != (B, 3, self.H, self.W) or out.image.device != dev:
            raise _lib.CavpError("FrameAugment: out= was made for other shapes")
        lib = _lib.load()
        st = C.c_void_p(_stream())
        jit = 0 if identity or self.jitter is None else 1
        if self.resize:
            return self._run_resize(lib, st, frames, masks, sizes, params, out, identity, jit, B, launches)
        if "plan" in launches:
            _lib.check(lib.cavp_aug_plan(_ptr(sizes), B, self.Hs, self.Ws, self.H, self.W, self._scales64, len(self.scales), jit,
                                         1 if identity else 0, _ptr(params), _ptr(state), _ptr(out.params), _ptr(self._near),
                                         _ptr(self._lsum), st), "cavp_aug_plan")
        if jit and "mean" in launches:
            _lib.check(lib.cavp_aug_contrast_mean(_ptr(frames), _ptr(sizes), B, self.Hs, self.Ws, max(self._scales64),
                                                  _ptr(out.params), _ptr(self._lsum), st), "cavp_aug_contrast_mean")
        if "render" in launches:
            _lib.check(lib.cavp_aug_render(_ptr(frames), _ptr(masks), _ptr(sizes), B, self.Hs, self.Ws, self.H, self.W, self._mean3,
                                           self._std3, self._fill3, jit, _ptr(out.params), _ptr(self._near), _ptr(self._lsum),
                                           _ptr(out.image), _ptr(out.label), st), "cavp_aug_render")
        self._last = out
        return out

    def _run_resize(self, lib, st, frames, masks, sizes, params, out, identity, jit, B, launches):
        """The resize variant's launches (module docstring); `launches` as in _run, with "store" for the scratch pass."""
        if identity and (self.Hs > RESIZE_MAX_RATIO * self.H or self.Ws > RESIZE_MAX_RATIO * self.W):
            raise _lib.CavpError(f"FrameAugment: eval_ with resize=True reduces by at most {RESIZE_MAX_RATIO} per axis: stage "
                                 f"{(self.Hs, self.Ws)} exceeds {RESIZE_MAX_RATIO} x crop {(self.H, self.W)}")
        state, smax = self._state, max(self._scales64)
        if "plan" in launches:
            _lib.check(lib.cavp_aug_plan_resize(_ptr(sizes), B, self.Hs, self.Ws, self.H, self.W, self._scales64, len(self.scales), jit,
                                                1 if identity else 0, _ptr(params), _ptr(state), _ptr(out.params), _ptr(self._near),
                                                _ptr(self._lsum), st), "cavp_aug_plan_resize")
        if jit and "mean" in launches:
            _lib.check(lib.cavp_aug_contrast_mean(_ptr(frames), _ptr(sizes), B, self.Hs, self.Ws, smax, _ptr(out.params),
                                                  _ptr(self._lsum), st), "cavp_aug_contrast_mean")
        if not identity and "store" in launches:
            _lib.check(lib.cavp_aug_resize_store(_ptr(frames), _ptr(sizes), B, self.Hs, self.Ws, smax, jit, _ptr(out.params),
                                                 _ptr(self._lsum), _ptr(self._scratch), st), "cavp_aug_resize_store")
        if "render" in launches:
            src = frames if identity else self._scratch
            _lib.check(lib.cavp_aug_resize_render(_ptr(src), 1 if identity else 0, _ptr(masks), _ptr(sizes), B, self.Hs, self.Ws, smax,
                                                  self.H, self.W, self._mean3, self._std3, _ptr(out.params), _ptr(self._near),
                                                  _ptr(out.image), _ptr(out.label), st), "cavp_aug_resize_render")
        self._last = out
        return out

    def __call__(self, frames: torch.Tensor, masks: torch.Tensor, sizes: torch.Tensor, params: Optional[torch.Tensor] = None,
                 out: Optional[AugResult] = None) -> AugResult:
        """params: int32 [B, 16] on the device, replaces the draws (PARAM_FIELDS; words 12..15 are ignored).
        out: a previous result of the same shapes whose buffers are written again (static addresses for a captured graph)."""
        return self._run(frames, masks, sizes, params, out, False)

    def eval_(self, frames: torch.Tensor, masks: torch.Tensor, sizes: torch.Tensor, out: Optional[AugResult] = None) -> AugResult:
        """The reference's test_aug (visual_aug.py:69-73): ToTensor + Normalize of the top-left H x W window, the mask widened to
        int64, through the render kernel with an identity plan (no draw is used, the offset still advances).  Where a staged
        frame is smaller than the window the rest is pad_fill / 255.  With resize=True: every frame and mask resized to H x W
        (BICUBIC / NEAREST) first, straight from the staged frames; needs stage_side <= 8 * crop_side."""
        return self._run(frames, masks, sizes, None, out, True)
