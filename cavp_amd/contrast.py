"""MI355X path of the reference's live contrastive loss, `loss/contrastive_aud.py::ContrastLoss` (SURVEY.md §8a row a13,
config #5).  Same constructor and `forward(embeds_match, gt_match, embeds_shuffle, gt_shuffle)`.

Split of work:
  host   - nearest-downsampling of the label maps and the class-balanced sampling (contrastive_aud.py:18-22,76-141):
           pure index bookkeeping on the (small) label tensors, done on the CPU with the SAME sequence of
           `torch.randperm` calls on the default CPU generator as the reference, so the sampled anchors are identical
           for an identical RNG state;
  device - L2-normalise + gather of the N anchors, S = A A^T / T on the f32 MFMA igemm, the row-wise InfoNCE, and the
           whole backward (dS, (dS + dS^T) A via the wgrad GEMM, normalisation backward, scatter into the feature
           gradient) - libcavp_hip.so only, no torch arithmetic.

Opt-in: `ContrastLoss.use_device_sampler(max_classes)` moves the sampling onto the device as well (same selection rule,
Philox4x32-10 keys instead of torch.randperm; include/cavp_hip.h ABI 14).  That path never touches the host between its
launches, so `loss = crit(...); loss.backward()` can be captured in a hipGraph.

Inside the native training step (`CAVP.train_step(contrast=crit, ...)`) the same chain runs without autograd on the tape's
compute-dtype NHWC fusion map: `NativeContrastTerm` at the end of this file (cavp_contrast_gather_nhwc / cavp_contrast_rows_bwd_add).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from . import train_ops as T
from .ops import _ptr, _stream


def nearest_indices(n_in: int, n_out: int) -> np.ndarray:
    """F.interpolate(mode='nearest') source index: min(floor(dst * float32(in / out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


# Host copies of down-sampled label maps, keyed by the label tensor's identity (+ version counter) and the target size.  The class-balanced
# sampling is index bookkeeping on the labels and runs on the host with the reference's own torch.randperm sequence; its only
# device dependency is this download.  Read inside the loss call it is a device-to-host copy on the launching stream: the host
# then waits for the whole forward pass that was queued in front of it, and the device idles while the host samples and launches
# (2.3 ms of an 18 ms config-#5 step in round 3).  Two ways out, both kept:
#   * `ContrastLoss.prefetch_labels(gt_match, gt_shuffle, size)` right after the batch reaches the device (before the model's
#     forward): the reduction + download run there, behind nothing, and the loss call finds the copy here;
#   * a label tensor OBJECT that was already downloaded and has not been written since (same object, same version counter) is
#     not downloaded again (validation-style loops over fixed batches, bench.py's synthetic step).
#     CONTRACT: the hit test is identity + torch's version counter, so it sees torch writes only.  A label buffer refilled behind
#     torch's back (a raw-pointer kernel, .data, a DLPack / numpy alias) must be followed by
#     invalidate_label_cache() before the next loss call (the returned arrays are read-only: callers never write into a cached copy).
_LABEL_CACHE: dict = {}
_LABEL_CACHE_MAX = 8


def invalidate_label_cache() -> None:
    """Forget every cached label download (see the contract above)."""
    _LABEL_CACHE.clear()


def _label_key(gt: torch.Tensor, size):
    return (id(gt), tuple(size))


def downsample_labels(gt: torch.Tensor, size: Tuple[int, int]) -> np.ndarray:
    """[B, H, W] int labels -> [B, h*w] (nearest).  Device labels are reduced ON the device (cavp_label_nearest) and only the
    B*h*w int32 result is downloaded for the host-side sampling (a 224 x 224 int64 batch is 16 x larger, a 512 x 512 one 84 x)."""
    if gt.is_cuda and gt.dim() == 3:
        # a hit needs the SAME tensor object (held through a weak reference: a new tensor the allocator placed at the old address
        # is another object), unwritten since (version counter)
        key = _label_key(gt, size)
        hit = _LABEL_CACHE.get(key)
        if hit is not None and hit[0]() is gt and hit[1] == gt._version:
            return hit[2]
        out = _downsample_labels_device(gt, size)
        out.setflags(write=False)   # the cached array is handed out by reference: a caller that wrote into it would poison later hits
        for k in [k for k, v in _LABEL_CACHE.items() if v[0]() is None]:
            del _LABEL_CACHE[k]
        if len(_LABEL_CACHE) >= _LABEL_CACHE_MAX:
            _LABEL_CACHE.pop(next(iter(_LABEL_CACHE)))
        _LABEL_CACHE[key] = (weakref.ref(gt), gt._version, out)
        return out
    g = gt.detach().cpu().numpy()
    hi, wi = nearest_indices(g.shape[1], size[0]), nearest_indices(g.shape[2], size[1])
    return g[:, hi][:, :, wi].reshape(g.shape[0], -1)


def _label_nearest_device(gt: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """[B, H, W] device labels -> int32 [B, h, w] on the device (cavp_label_nearest); no host involvement."""
    g = gt.detach()
    if g.dtype != torch.int64 or not g.is_contiguous():
        g = g.to(torch.int64).contiguous()
    out = torch.empty((g.shape[0], size[0], size[1]), dtype=torch.int32, device=g.device)
    _lib.check(_lib.load().cavp_label_nearest(_ptr(g), _ptr(out), g.shape[0], g.shape[1], g.shape[2], size[0], size[1],
                                              C.c_void_p(_stream())), "cavp_label_nearest")
    return out


def _downsample_labels_device(gt: torch.Tensor, size: Tuple[int, int]) -> np.ndarray:
    out = _label_nearest_device(gt, size)
    return out.cpu().numpy().astype(np.int64).reshape(out.shape[0], -1)


_PINNED: dict = {}


def _upload_i32(arrs, dev):
    """Several small int32 host arrays -> one device tensor through a PINNED staging buffer (a pageable torch.from_numpy().to(dev)
    is a blocking copy each); returns the device views.  One staging buffer per call slot (two rotate) so that a copy still in
    flight is not overwritten by the next step's indices."""
    n = sum(int(a.size) for a in arrs)
    # staging slots per (device, thread): nn.DataParallel replica threads and loss calls on different devices must not share one
    # (the event is recorded after the host writes, so a second user of the slot could overwrite a buffer whose copy is pending)
    import threading
    own = _PINNED.setdefault((torch.device(dev).index or 0, threading.get_ident()), {})
    slot = own.get("slot", 0)
    own["slot"] = slot ^ 1
    buf, ev = own.get(slot, (None, None))
    if ev is not None:
        ev.synchronize()       # the copy that last used this staging buffer has run (two steps ago: normally long done)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1 << 14), dtype=torch.int32).pin_memory()
    views, o = [], 0
    host = buf.numpy()
    for a in arrs:
        host[o:o + a.size] = a.reshape(-1)
        o += a.size
    d = buf[:n].to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    own[slot] = (buf, ev)
    o = 0
    for a in arrs:
        views.append(d[o:o + a.size])
        o += a.size
    return views


class SamplePlan:
    """Anchors chosen by `extraction_samples`: first `n_match` rows come from embeds_match, the rest from embeds_shuffle."""
    __slots__ = ("b", "p", "labels", "n_match", "n")

    def __init__(self, b, p, labels, n_match):
        self.b, self.p, self.labels, self.n_match, self.n = b, p, labels, n_match, len(b)


def sample_anchors(gt_match: np.ndarray, gt_shuffle: np.ndarray, ignore_idx: int, max_views: int) -> Optional[SamplePlan]:
    """contrastive_aud.py:76-141 on [B, hw] label arrays; consumes torch.randperm exactly like the reference."""
    B, HW = gt_match.shape
    # flat pixel indices throughout; (image, pixel) only for the few hundred anchors that are kept (the first version split all
    # B * hw indices and gathered three B * hw-sized arrays per call: 4 of the 6 ms this function cost per step at B = 30)
    gm = gt_match.reshape(-1)
    fg_idx = np.flatnonzero((gm > 0) & (gm != ignore_idx))
    fg_l = gm[fg_idx]
    sel: List[np.ndarray] = []
    sel_l: List[np.ndarray] = []
    for item in np.unique(fg_l):                       # torch.unique: sorted ascending
        cur = np.flatnonzero(fg_l == item)
        if cur.shape[0] < max_views:
            continue
        r = torch.randperm(cur.shape[0]).numpy()[:max_views]
        sel.append(fg_idx[cur[r]]); sel_l.append(fg_l[cur[r]])
    if not sel:
        return None
    bg_idx = np.flatnonzero(gm == 0)
    sample_num = int(min(max_views, fg_idx.shape[0], bg_idx.shape[0]))
    i1 = torch.randperm(bg_idx.shape[0]).numpy()[:sample_num]
    i2 = torch.randperm(fg_idx.shape[0]).numpy()[:sample_num]
    idx = np.concatenate(sel + [bg_idx[i1], fg_idx[i2]])
    # shuffle-branch candidates live at the MATCH foreground pixels
    lab = np.concatenate(sel_l + [np.zeros(sample_num, dtype=gm.dtype), gt_shuffle.reshape(-1)[fg_idx[i2]]])
    b, p = np.divmod(idx, HW)
    return SamplePlan(b.astype(np.int32), p.astype(np.int32), lab.astype(np.int32), len(idx) - sample_num)


def _strides_bcp(x: torch.Tensor) -> Tuple[int, int, int]:
    """element strides (batch, channel, pixel) of a [B, C, H, W] tensor whose (H, W) plane is a uniform pixel grid."""
    sb, sc, sh, sw = x.stride()
    if x.shape[3] > 1 and x.shape[2] > 1 and sh != sw * x.shape[3]:
        raise _lib.CavpError("feature map must have a uniform pixel stride (NCHW-contiguous or channels-last)")
    return sb, sc, sw


class DevicePlan:
    """What the device sampler chose in one call; every field is a device tensor.  header: int32[8] = {n, n_match, k_kept,
    sample_num, offset_lo, offset_hi, seed_lo, seed_hi}; idx_b / idx_p / labels: int32[cap] (rows >= n hold -1)."""
    __slots__ = ("header", "idx_b", "idx_p", "labels", "cap", "work", "gm", "gs")

    def __init__(self, header, idx_b, idx_p, labels, cap, work, gm, gs):
        self.header, self.idx_b, self.idx_p, self.labels, self.cap, self.work, self.gm, self.gs = \
            header, idx_b, idx_p, labels, cap, work, gm, gs


def sample_anchors_device(gm: torch.Tensor, gs: torch.Tensor, ignore_idx: int, max_views: int, max_classes: int,
                          state: torch.Tensor) -> DevicePlan:
    """cavp_contrast_sample on the reduced int32 label maps [B, h, w]: three launches, nothing read by the host.  `state` is the
    sampler's persistent int64[4] = {seed, offset, dropped_classes, bad_labels}."""
    lib = _lib.load()
    dev = gm.device
    total, hw = gm.numel(), gm.shape[1] * gm.shape[2]
    cap = (max_classes + 2) * max_views
    # one allocation: header | idx_b | idx_p | labels; the kernels' scratch in a second one
    buf = torch.empty(8 + 3 * cap, dtype=torch.int32, device=dev)
    header, ib, ip, lab = buf[:8], buf[8:8 + cap], buf[8 + cap:8 + 2 * cap], buf[8 + 2 * cap:]
    work = torch.empty(lib.cavp_contrast_sample_work_bytes(max_classes) // 4, dtype=torch.int32, device=dev)
    _lib.check(lib.cavp_contrast_sample(_ptr(gm), _ptr(gs), total, hw, int(ignore_idx), max_views, max_classes, _ptr(state),
                                        _ptr(header), _ptr(work), _ptr(ib), _ptr(ip), _ptr(lab), C.c_void_p(_stream())),
               "cavp_contrast_sample")
    return DevicePlan(header, ib, ip, lab, cap, work, gm, gs)


class _PlanArgs(NamedTuple):
    """What a launch of the chain needs, for either plan type.  header None: the count is the host's (n, n_match), cap 0; else the
    count is read from the header on the device and n = n_match = 0.  npad: the row count of A / S."""
    header: Optional[torch.Tensor]
    idx_b: torch.Tensor
    idx_p: torch.Tensor
    labels: Optional[torch.Tensor]
    cap: int
    n: int
    n_match: int
    npad: int


def _plan_args(plan, dev=None, idx=None) -> _PlanArgs:
    """A SamplePlan's three arrays are uploaded to `dev` here (once per step: the chain keeps the result).  A caller that holds the
    index arrays on the device already passes idx = (idx_b, idx_p) and gets no labels."""
    if isinstance(plan, DevicePlan):
        return _PlanArgs(plan.header, plan.idx_b, plan.idx_p, plan.labels, plan.cap, 0, 0, (plan.cap + 3) // 4 * 4)
    if idx is not None:
        ib, ip, lab = idx[0], idx[1], None
    elif dev is not None:
        ib, ip, lab = _upload_i32((plan.b, plan.p, plan.labels), dev)
    else:
        raise _lib.CavpError("a SamplePlan needs its index arrays on the device: idx = (idx_b, idx_p)")
    return _PlanArgs(None, ib, ip, lab, 0, plan.n, plan.n_match, (plan.n + 3) // 4 * 4)


def _infonce_from_rows(A: torch.Tensor, pa: _PlanArgs, temperature: float, eps: float, need_grad: bool = True):
    """The middle of the chain on the filled A [npad, C]: S = A A^T / T on the f32 MFMA path, the InfoNCE rows, loss (f32 [1]) and,
    with need_grad, dS = dloss / dS.  Returns (S, rows, loss, dS)."""
    dev, (npad, Cc) = A.device, A.shape
    S = torch.empty((npad, npad), dtype=torch.float32, device=dev)
    inv_t = torch.full((npad,), 1.0 / temperature, dtype=torch.float32, device=dev)
    ops.linear(A, A.view(npad, 1, 1, Cc), S, scale=inv_t)
    rows = torch.empty(npad, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dS = torch.empty_like(S) if need_grad else None
    _lib.check(_lib.load().cavp_infonce_rows(_ptr(S), _ptr(pa.labels), _ptr(pa.header), pa.cap, pa.n, npad, C.c_float(eps), _ptr(rows),
                                             _ptr(loss), _ptr(dS), C.c_float(1.0), C.c_void_p(_stream())), "cavp_infonce_rows")
    return S, rows, loss, dS


def _rows_grad(dS: torch.Tensor, A: torch.Tensor, scale: float, scale_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dA = scale * scale_dev[0] * (dS + dS^T) A  (anchors and contrasts are the same tensor: both roles get gradient).  scale_dev is
    a device scalar, multiplied in on the device - float(gout) made the host wait for the whole forward + loss queue before it
    could launch the backward."""
    G = torch.empty_like(dS)
    _lib.check(_lib.load().cavp_symm_add(_ptr(dS), _ptr(G), dS.shape[0], C.c_float(scale), _ptr(scale_dev), C.c_void_p(_stream())),
               "cavp_symm_add")
    dA = T.zeros(tuple(A.shape), torch.float32, A.device)
    T.linear_wgrad(A, G, dA)
    return dA


class _InfoNCEFn(torch.autograd.Function):
    """The loss on the f32 feature maps [B, C, h, w] (any uniform pixel stride) for a SamplePlan or a DevicePlan.  With a DevicePlan
    every buffer has the static capacity of the plan and the kernels read n and n_match from the plan header: no host decision
    depends on a device value, in either direction."""

    @staticmethod
    def forward(ctx, em, es, plan, temperature: float, eps: float):
        pa = _plan_args(plan, em.device)
        Cc = em.shape[1]
        A = torch.empty((pa.npad, Cc), dtype=torch.float32, device=em.device)    # the kernel writes the padding rows
        norms = torch.empty(pa.npad, dtype=torch.float32, device=em.device)
        _lib.check(_lib.load().cavp_gather_l2norm(_ptr(em), *_strides_bcp(em), _ptr(es), *_strides_bcp(es), _ptr(pa.header),
                                                  _ptr(pa.idx_b), _ptr(pa.idx_p), pa.cap, pa.n, pa.n_match, pa.npad, Cc,
                                                  C.c_float(1e-12), _ptr(A), _ptr(norms), C.c_void_p(_stream())), "cavp_gather_l2norm")
        _, _, loss, dS = _infonce_from_rows(A, pa, temperature, eps, em.requires_grad or es.requires_grad)
        ctx.saved = (A, norms, dS, pa, em.shape, es.shape, temperature)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        A, norms, dS, pa, em_shape, es_shape, temperature = ctx.saved
        dA = _rows_grad(dS, A, 1.0 / temperature, gout.detach().reshape(1).to(torch.float32))
        # NHWC memory, cleared by a launch; NCHW views are returned
        gm, gs = (T.zeros((b, h, w, c), torch.float32, A.device) for b, c, h, w in (em_shape, es_shape))
        _lib.check(_lib.load().cavp_l2norm_bwd_scatter(_ptr(dA), _ptr(A), _ptr(norms), _ptr(pa.header), _ptr(pa.idx_b), _ptr(pa.idx_p),
                                                       pa.cap, pa.n, pa.n_match, A.shape[1], _ptr(gm), *_strides_bcp(gm.permute(0, 3, 1, 2)), _ptr(gs),
                                                       *_strides_bcp(gs.permute(0, 3, 1, 2)), C.c_void_p(_stream())),
                   "cavp_l2norm_bwd_scatter")
        return gm.permute(0, 3, 1, 2), gs.permute(0, 3, 1, 2), None, None, None


class ContrastLoss(nn.Module):
    def __init__(self, temperature, ignore_idx, max_views):
        super().__init__()
        self.ignore_idx = ignore_idx
        self.ood_idx = 254
        self.eps = 1e-12
        self.temperature = temperature
        self.max_views = max_views
        self._dev = None           # device sampler: (max_classes, state int64[4]) once use_device_sampler() was called
        self._last_plan = None

    # ---- opt-in device-side sampling -------------------------------------------------------------------------------------
    def use_device_sampler(self, max_classes: int, seed: int = 0, *, device=None) -> "ContrastLoss":
        """Switch this instance to the device sampler: the class-balanced selection of contrastive_aud.py:76-141 with
        Philox4x32-10 keys in place of torch.randperm (same distribution, another stream: the anchors differ from the host
        sampler's and from the reference's for any seed).  After this call forward() and backward() make no device-to-host copy,
        no host-to-device copy and no stream synchronisation and allocate through torch's caching allocator only, so
        `with torch.cuda.graph(g): loss = crit(em, gt, es, gs); loss.backward()` works (after one eager warm-up call, which sizes
        the GEMM workspace).  Every replay draws fresh anchors: the call counter lives on the device.

        max_classes: the largest number of foreground classes that may qualify (>= max_views pixels) in one batch.  It fixes the
        static anchor capacity Ncap = (max_classes + 2) * max_views at which the GEMMs run.  If more classes qualify, the
        lowest-numbered max_classes are kept and the device counter `dropped_classes` grows by the surplus (last_plan()).

        Differences from the default path: the loss is always 0-dim; when no class qualifies its value is 0 and both feature
        gradients are zero (the reference returns a constant of shape [1] there - a shape cannot follow a device value without
        a synchronisation).  Labels must lie in [0, 255]: the host cannot look at them without a copy, so the count kernel
        counts the ones outside (they belong to no group) and last_plan() raises CavpError when there were any."""
        if not isinstance(max_classes, int) or not 1 <= max_classes <= 254:
            raise _lib.CavpError("use_device_sampler: 1 <= max_classes <= 254")
        if not isinstance(self.max_views, int) or not 1 <= self.max_views <= 1024:
            raise _lib.CavpError("the device sampler needs 1 <= max_views <= 1024")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._dev = (max_classes, torch.zeros(4, dtype=torch.int64, device=dev))
        self._last_plan = None
        self.manual_seed(seed)
        return self

    def manual_seed(self, seed: int) -> None:
        """Reset the device sampler's seed and its call counter (offset 0).  A host-to-device write: not legal while a hipGraph
        is being captured; graphs captured earlier see the new values on their next replay."""
        if self._dev is None:
            raise _lib.CavpError("manual_seed: call use_device_sampler() first (the host sampler follows torch.manual_seed)")
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        s = s - (1 << 64) if s >= (1 << 63) else s
        self._dev[1][:2].copy_(torch.tensor([s, 0], dtype=torch.int64))

    def rollback_ranges(self):
        """[(name, tensor, byte_offset, nbytes)]: {seed, offset} of the device sampler's int64[4], the state a call mutates (the
        dropped-class and bad-label counters behind them are diagnostics and are not named).  For
        cavp_amd.rollback.StepRollback.add()."""
        if self._dev is None:
            raise _lib.CavpError("rollback_ranges: call use_device_sampler() first (the host sampler keeps no device state)")
        return [("state", self._dev[1], 0, 16)]

    def last_plan(self) -> dict:
        """The device tensors of the most recent device-sampler call (of the captured call, after a graph replay): `header`
        int32[4] = {n, n_match, k_eligible (classes kept), sample_num}, `idx_b`, `idx_p`, `labels` (int32[Ncap], rows >= n hold
        -1), `dropped_classes` (int64[1], cumulative), `seed_offset` (int32[4]: the offset and seed this call drew with, low /
        high words).  For tests and debugging: it reads the bad-label counter, which synchronises - never call it in a capture.
        Raises CavpError if a label outside [0, 255] was seen since the last check."""
        if self._dev is None or self._last_plan is None:
            raise _lib.CavpError("last_plan: no device-sampler call yet")
        state, p = self._dev[1], self._last_plan
        bad = int(state[3].item())
        if bad:
            state[3:4].zero_()
            raise _lib.CavpError(f"ContrastLoss device sampler: {bad} label(s) outside [0, 255]")
        return {"header": p.header[:4], "idx_b": p.idx_b, "idx_p": p.idx_p, "labels": p.labels,
                "dropped_classes": state[2:3], "seed_offset": p.header[4:8]}

    def _forward_device(self, embeds_match, gt_match, embeds_shuffle, gt_shuffle):
        max_classes, state = self._dev
        em, es = embeds_match, embeds_shuffle
        if em.device != state.device:
            raise _lib.CavpError(f"device sampler lives on {state.device}, features on {em.device}")
        if em.dim() != 4 or em.shape != es.shape:
            raise _lib.CavpError("ContrastLoss: embeds_match and embeds_shuffle must be [B, C, h, w] of one shape")
        B, _, h, w = em.shape
        if B * h * w >= 2 ** 31:
            raise _lib.CavpError("the device sampler needs B*h*w < 2**31")
        if not isinstance(self.max_views, int) or not 1 <= self.max_views <= 1024:
            raise _lib.CavpError("the device sampler needs 1 <= max_views <= 1024")
        for g in (gt_match, gt_shuffle):
            if not g.is_cuda or g.dim() != 3 or g.shape[0] != B or g.is_floating_point() or g.dtype == torch.bool:
                raise _lib.CavpError("the device sampler needs integer [B, H, W] label maps on the device")
        _strides_bcp(em), _strides_bcp(es)
        plan = sample_anchors_device(_label_nearest_device(gt_match, (h, w)), _label_nearest_device(gt_shuffle, (h, w)),
                                     self.ignore_idx, self.max_views, max_classes, state)
        self._last_plan = plan
        return _InfoNCEFn.apply(em, es, plan, float(self.temperature), float(self.eps))

    @staticmethod
    def prefetch_labels(gt_match, gt_shuffle, size) -> None:
        """Optional, for trainers: call right after the batch is on the device (before the model's forward) with the spatial size
        of the feature map the loss will see (out_fusion: H/4 x W/4).  The label reduction and its download then do not wait
        behind the forward pass; forward() finds the host copies by the tensors' identity + version."""
        for g in (gt_match, gt_shuffle):
            downsample_labels(g, tuple(size))

    def forward(self, embeds_match, gt_match, embeds_shuffle, gt_shuffle):
        if not embeds_match.is_cuda:
            raise _lib.CavpError("ContrastLoss (MI355X path) needs HIP device tensors: there is no CPU fallback")
        if embeds_match.dtype != torch.float32 or embeds_shuffle.dtype != torch.float32:
            raise _lib.CavpError("ContrastLoss expects the f32 out_fusion features")
        if self._dev is not None:
            return self._forward_device(embeds_match, gt_match, embeds_shuffle, gt_shuffle)
        size = tuple(embeds_match.shape[2:])
        plan = sample_anchors(downsample_labels(gt_match, size), downsample_labels(gt_shuffle, size), self.ignore_idx,
                              self.max_views)
        if plan is None:
            return torch.tensor([0.0], device=gt_match.device)          # contrastive_aud.py:35-36
        return _InfoNCEFn.apply(embeds_match, embeds_shuffle, plan, float(self.temperature), float(self.eps))


# ---- the loss on the training tape's fusion map (CAVP.train_step(contrast=...)) ---------------------------------------------------
def anchor_rows(idx_b, idx_p, n_match: int, B: int, hw: int) -> np.ndarray:
    """Row of each anchor in the tape's fusion map viewed as [2B * hw, ld]: image idx_b[i] of the match half for i < n_match, image
    B + idx_b[i] of the shuffle half after it (the addressing of cavp_contrast_gather_nhwc / cavp_contrast_rows_bwd_add)."""
    b, p = np.asarray(idx_b, dtype=np.int64), np.asarray(idx_p, dtype=np.int64)
    if b.shape != p.shape or b.ndim != 1 or not 0 <= n_match <= b.shape[0]:
        raise _lib.CavpError("anchor_rows: idx_b / idx_p must be 1-d of one length, 0 <= n_match <= their length")
    if b.size and (b.min() < 0 or b.max() >= B or p.min() < 0 or p.max() >= hw):
        raise _lib.CavpError("anchor_rows: an anchor lies outside the [B] x [hw] map")
    half = (np.arange(b.shape[0]) >= n_match).astype(np.int64)
    return (b + half * B) * hw + p


def _nhwc_map_args(x: torch.Tensor, what: str):
    """(B, hw, ld, C) of a fusion map [2B, h, w, C] (or [2B, hw, C]) whose pixels are ld elements apart; raises on anything else."""
    if not x.is_cuda:
        raise _lib.CavpError(f"{what}: needs a HIP device tensor (there is no CPU fallback)")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.CavpError(f"{what}: float32 or bfloat16 map required, got {x.dtype}")
    if x.dim() not in (3, 4) or x.shape[0] % 2 or x.stride(-1) != 1:
        raise _lib.CavpError(f"{what}: [2B, h, w, C] map with unit channel stride required, got shape {tuple(x.shape)}")
    n2, Cc, ld = x.shape[0], x.shape[-1], x.stride(-2)
    hw = x.numel() // (n2 * Cc)
    dense = x.stride(0) == hw * ld and (x.dim() == 3 or x.shape[2] == 1 or x.stride(1) == x.shape[2] * ld)
    if not dense or ld < Cc:
        raise _lib.CavpError(f"{what}: pixels must lie ld elements apart throughout, got strides {x.stride()}")
    if Cc % 8:
        raise _lib.CavpError(f"{what}: channel width {Cc} is not a multiple of 8")
    return n2 // 2, hw, ld, Cc


def contrast_gather_nhwc(x: torch.Tensor, plan, idx, A: torch.Tensor, norms: torch.Tensor, eps: float = 1e-12) -> None:
    """A[i] = x_row / max(||x_row||, eps) (f32 [rows, C]) and norms[i] for the plan's anchors, read from the map in its own dtype."""
    B, hw, ld, Cc = _nhwc_map_args(x, "contrast_gather_nhwc")
    if A.dtype != torch.float32 or norms.dtype != torch.float32 or not A.is_contiguous() or A.shape[1] != Cc or norms.numel() < A.shape[0]:
        raise _lib.CavpError("contrast_gather_nhwc: A must be dense f32 [rows, C] with one norm per row")
    pa = _plan_args(plan, idx=idx)
    _lib.check(_lib.load().cavp_contrast_gather_nhwc(ops.dtype_code(x.dtype), _ptr(x), B, hw, ld, Cc, _ptr(pa.header), _ptr(pa.idx_b),
                                                     _ptr(pa.idx_p), pa.cap, pa.n, pa.n_match,
                                                     A.shape[0], C.c_float(eps), _ptr(A), _ptr(norms), C.c_void_p(_stream())),
               "cavp_contrast_gather_nhwc")


def contrast_rows_bwd_add(g: torch.Tensor, plan, idx, dA: torch.Tensor, A: torch.Tensor, norms: torch.Tensor, scale: float = 1.0) -> None:
    """g_row += scale * (dA_i - A_i <A_i, dA_i>) / norms[i] for the plan's anchors, in place in the map's own dtype."""
    B, hw, ld, Cc = _nhwc_map_args(g, "contrast_rows_bwd_add")
    for t in (dA, A):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != Cc:
            raise _lib.CavpError("contrast_rows_bwd_add: A / dA must be dense f32 [rows, C]")
    pa = _plan_args(plan, idx=idx)
    if min(A.shape[0], dA.shape[0], norms.numel()) < (pa.cap if pa.header is not None else pa.n):
        raise _lib.CavpError("contrast_rows_bwd_add: A / dA / norms hold fewer rows than the plan")
    _lib.check(_lib.load().cavp_contrast_rows_bwd_add(ops.dtype_code(g.dtype), _ptr(g), B, hw, ld, Cc, _ptr(pa.header), _ptr(pa.idx_b),
                                                      _ptr(pa.idx_p), pa.cap, pa.n, pa.n_match,
                                                      _ptr(dA), _ptr(A), _ptr(norms), C.c_float(scale), C.c_void_p(_stream())),
               "cavp_contrast_rows_bwd_add")


class NativeContrastTerm:
    """The contrast term of one native training step (CAVP.train_step(contrast=crit)), without autograd and without a tensor of the
    fusion map's size: labels -> plan -> gather from the compute-dtype NHWC map -> S -> InfoNCE -> dA, and `add_rows`, the gradient
    tap that adds the anchors' rows into the map's gradient.  Three calls, in the order the step makes them:
      __init__   both label maps reduced to `size` on the device; device sampler: the plan (three launches); host sampler: the
                 download of the reduced labels - before any model kernel is queued, so it waits behind nothing;
      draw()     host sampler: the torch.randperm draws, in the reference's order (after the forward, whose DropPath may draw too);
      run()      the chain up to dA on the finished map; returns the unweighted loss, f32 [1] on the device."""

    def __init__(self, crit: "ContrastLoss", label: torch.Tensor, label_shuffle: torch.Tensor, size: Tuple[int, int]):
        for g in (label, label_shuffle):
            if not g.is_cuda or g.dim() != 3 or g.is_floating_point() or g.dtype == torch.bool:
                raise _lib.CavpError("train_step(contrast=...): integer [B, H, W] label maps on the device required")
        if label.shape != label_shuffle.shape:
            raise _lib.CavpError(f"train_step(contrast=...): label {tuple(label.shape)} and label_shuffle "
                                 f"{tuple(label_shuffle.shape)} differ in shape")
        self.crit, self.size, self.plan, self.saved = crit, tuple(size), None, None
        self._host = None
        if crit._dev is not None:
            max_classes, state = crit._dev
            if state.device != label.device:
                raise _lib.CavpError(f"device sampler lives on {state.device}, labels on {label.device}")
            if label.shape[0] * size[0] * size[1] >= 2 ** 31:
                raise _lib.CavpError("the device sampler needs B*h*w < 2**31")
            self.plan = sample_anchors_device(_label_nearest_device(label, self.size), _label_nearest_device(label_shuffle, self.size),
                                              crit.ignore_idx, crit.max_views, max_classes, state)
            crit._last_plan = self.plan
        else:
            self._host = (downsample_labels(label, self.size), downsample_labels(label_shuffle, self.size))

    def draw(self) -> None:
        if self._host is not None:
            self.plan = sample_anchors(self._host[0], self._host[1], self.crit.ignore_idx, self.crit.max_views)   # None: no class qualifies

    def run(self, fusion: torch.Tensor, grad_scale: float) -> torch.Tensor:
        """fusion: the tape's map [2B, h, w, C].  grad_scale: d(total loss) / d(this term).  Leaves what add_rows needs."""
        dev = fusion.device
        if tuple(fusion.shape[1:3]) != self.size:
            raise _lib.CavpError(f"train_step(contrast=...): the fusion map is {tuple(fusion.shape[1:3])}, the labels were reduced to {self.size}")
        plan = self.plan
        if plan is None:
            return T.zeros((1,), torch.float32, dev)
        pa = _plan_args(plan, dev)
        idx = (pa.idx_b, pa.idx_p)
        A = torch.empty((pa.npad, fusion.shape[-1]), dtype=torch.float32, device=dev)
        norms = torch.empty(pa.npad, dtype=torch.float32, device=dev)
        contrast_gather_nhwc(fusion, plan, idx, A, norms)
        _, _, loss, dS = _infonce_from_rows(A, pa, self.crit.temperature, float(self.crit.eps))
        dA = _rows_grad(dS, A, grad_scale / self.crit.temperature)
        self.saved = (plan, idx, dA, A, norms)
        return loss

    def add_rows(self, g: torch.Tensor) -> bool:
        """TrainPass.grad_tap function of the fusion map."""
        if self.saved is None:
            return False
        plan, idx, dA, A, norms = self.saved
        contrast_rows_bwd_add(g, plan, idx, dA, A, norms, 1.0)
        return True
