"""Training pass of the CAVP hot path on MI355X: forward with batch-statistics BatchNorm + hand-written backward.

The reference trains through torch.autograd over stock modules (trainer_cavp_vpo_mono.py:168-193).  Here the whole
model is ONE autograd node (`CAVPTrainFunction`): its forward runs the HIP kernels and records a tape of backward
closures over the saved NHWC activations; its backward replays the tape (dgrad = the same MFMA implicit-GEMM on
rot180/transposed weights, wgrad = the pixel-reduction MFMA GEMM, BN/LN/GELU/pool/resize backward kernels) and hands
torch one f32 gradient per parameter, so the reference's losses / optimisers / DDP hooks run unchanged on top.

Semantics kept from the reference:
  * BatchNorm uses batch statistics when its module is in training mode and updates running_mean / running_var /
    num_batches_tracked (momentum 0.1, unbiased variance); nn.SyncBatchNorm modules all-reduce their statistics over
    torch.distributed (RCCL) when a process group is initialised (main_vpo_mono.py:130).
  * forward_train duplicates the visual features to 2B (cavp_model.py:181) and runs audio / fusion / decoder on 2B.
  * parameters that receive no gradient in the reference (pos_embed_*, audio_backbone.cls_head) get None.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from . import train_ops as T
from ._lib import ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_RELU, CavpError
from ._lib import load as _lib_load


class V:
    """An activation (NHWC / token / vector tensor) and its gradient.  A channel slice of a wider buffer is a child
    whose gradient is the matching slice of the parent's gradient (free concat in both directions)."""
    __slots__ = ("t", "_g", "parent", "lo", "hi", "needs_grad", "tile_stats", "grad_mul", "g_premul", "dp_scale", "g_scaled",
                 "bnb", "bnb_claim", "bnb_part")

    def __init__(self, t: torch.Tensor, parent: Optional["V"] = None, lo: int = 0, hi: int = 0, needs_grad: bool = True):
        self.t, self._g, self.parent, self.lo, self.hi, self.needs_grad = t, None, parent, lo, hi, needs_grad
        self.tile_stats = None   # (buf, tiles, rows_per_tile) when the producing conv computed BN statistics
        # fused fc1 + GELU (TrainPass.conv(act=ACT_GELU)): the gelu' tensor the producer of this activation's gradient multiplies
        # into its epilogue, and whether .g already carries that factor
        self.grad_mul, self.g_premul = None, False
        # output of `x + DropPath(branch)`: the per-image factor of the branch, and - when the LAST contributor to .g was a
        # LayerNorm backward - the branch's gradient factor * .g, written by that kernel as a second output (any later
        # accumulation into .g drops it again)
        self.dp_scale, self.g_scaled = None, None
        # output of a local train-mode BatchNorm (+ residual) + ReLU (TrainPass.bn_act): what the data-gradient launch that completes
        # this activation's gradient needs to fold the BatchNorm backward's two reductions into its epilogue (bnb), the first consumer
        # in forward order = the last contributor in the backward (bnb_claim: that conv's token, or False), and - while .g is exactly
        # what that launch wrote - its per-tile partial sums (bnb_part; any later accumulation into .g drops them)
        self.bnb, self.bnb_claim, self.bnb_part = None, None, None

    @property
    def g(self) -> Optional[torch.Tensor]:
        if self.parent is not None:
            pg = self.parent.g
            return None if pg is None else pg[..., self.lo:self.hi]
        return self._g

    def set_g(self, g: torch.Tensor) -> None:
        if self.parent is not None:
            raise CavpError("gradient of a slice is owned by its parent")
        self._g = g
        self.g_scaled = None
        self.bnb_part = None

    def slice(self, lo: int, hi: int) -> "V":
        return V(self.t[..., lo:hi], parent=self, lo=lo, hi=hi)


def _as4(t: torch.Tensor) -> torch.Tensor:
    if t.dim() == 4:
        return t
    if t.dim() == 3:
        return t.unsqueeze(1)
    if t.dim() == 2:
        return t.unsqueeze(1).unsqueeze(1)
    raise CavpError("expected a 2/3/4-d activation")


class _P:
    """Kernel-ready parameters of one conv / linear for the training pass."""
    __slots__ = ("w", "wT", "weight", "bias", "kh", "kw", "stride", "pad", "dil", "cout", "cin", "real_weight",
                 "real_bias", "real_cout")


class GradArena:
    """One flat f32 buffer holding every parameter gradient (views per parameter): a single memset per step and a
    single RCCL all-reduce over xGMI for data parallelism (C1 in SURVEY.md §2.3) instead of one per tensor/bucket."""

    def __init__(self, params, device, late_ids=None, no_zero_ids=None):
        """`late_ids`: ids of the parameters whose gradients become final LAST in the backward pass (backbone, ASPP,
        low-level reduce).  They are laid out first, so that `flat[split:]` - everything the backward finishes early
        (decoder head, cross attention, projector, the 73 M-parameter audio encoder = ~75 % of the bytes) - is one
        contiguous range that can be all-reduced while the rest of the backward still runs."""
        ps = [p for p in params if p.requires_grad]
        late_ids = late_ids or set()
        self.params = [p for p in ps if id(p) in late_ids] + [p for p in ps if id(p) not in late_ids]
        total = sum((p.numel() + 3) // 4 * 4 for p in self.params)   # keep every view 16-byte aligned
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.views: Dict[int, torch.Tensor] = {}
        # `no_zero_ids`: large weights whose first gradient contribution of a step OVERWRITES the view (beta = 0 weight-
        # gradient GEMM, TrainPass._wgrad): they are left out of the per-step memset (the 12288 x 4096 audio fc alone is a
        # 201 MB clear + a 201 MB read-modify-write otherwise).  TrainPass clears such a view itself if its first touch comes
        # from any other path.
        self.no_zero = set(no_zero_ids or ())
        off = 0
        self.split = 0
        ranges, start = [], 0   # [start, end) element ranges that zero() clears
        for p in self.params:
            if id(p) in late_ids:
                self.split = off + (p.numel() + 3) // 4 * 4
            self.views[id(p)] = self.flat[off:off + p.numel()].view(p.shape)
            if id(p) in self.no_zero:
                if off > start:
                    ranges.append((start, off))
                start = off + (p.numel() + 3) // 4 * 4
            off += (p.numel() + 3) // 4 * 4
        if off > start:
            ranges.append((start, off))
        self._zero_ranges = ranges
        self._zero_table = (torch.tensor([v for r in ranges for v in r], dtype=torch.int64).to(device)
                            if ranges and self.flat.is_cuda else None)

    def zero(self) -> None:
        """One launch for all ranges (about 30 when the big weights are overwritten instead of cleared)."""
        if self._zero_table is None:
            for a, b in self._zero_ranges:
                self.flat[a:b].zero_()     # CPU arena of the gloo plumbing tests
            return
        T._check(_lib_load().cavp_zero_ranges_f32(T._ptr(self.flat), T._ptr(self._zero_table), len(self._zero_ranges),
                                                  max(b - a for a, b in self._zero_ranges), T._s()), "cavp_zero_ranges_f32")


def dist_world() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


# True (tests only): issue the gradient collectives even in a process group of ONE rank, so that the real RCCL backend, its
# streams and its interplay with the hipGraph replays are exercised on a single-GPU box (tests/test_gpu_nccl_world1.py).
FORCE_COLLECTIVES = False


def collectives_on() -> bool:
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or FORCE_COLLECTIVES)


# Wire format of the gradient all-reduce.  f32 (default) = the reference's DDP (main_vpo_mono.py:131-135: 479 MB per step).
# bf16 (opt-in, `set_grad_allreduce_dtype(torch.bfloat16)`, `bench.py --grad-allreduce bf16`): each piece is cast into a bf16
# staging buffer, summed over the ranks in bf16 and cast back - 240 MB on the xGMI links instead of 479 MB (SURVEY.md section 5:
# a ring all-reduce is bound by ONE link's ~153 GB/s); the arena and the optimiser stay f32.  Every rank's contribution is
# rounded to bf16 once and the partial sums are rounded on the way round the ring (relative error ~ 2^-8 per element).
_GRAD_WIRE_DTYPE = torch.float32


def set_grad_allreduce_dtype(dtype: torch.dtype) -> None:
    global _GRAD_WIRE_DTYPE
    if dtype not in (torch.float32, torch.bfloat16):
        raise CavpError("gradient all-reduce wire format: torch.float32 or torch.bfloat16")
    _GRAD_WIRE_DTYPE = dtype


def grad_allreduce_dtype() -> torch.dtype:
    return _GRAD_WIRE_DTYPE


def _convert(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dtype conversion of a flat range: the HIP cast kernel on the device, a torch copy for the CPU arenas of the gloo tests."""
    if src.is_cuda:
        return ops.cast(src, dst)
    return dst.copy_(src)


class _WireWork:
    """An in-flight piece of the compressed all-reduce: the collective's handle + the cast back into the f32 arena."""

    def __init__(self, work, wire: torch.Tensor, dst: torch.Tensor):
        self.work, self.wire, self.dst = work, wire, dst

    def wait(self) -> None:
        if self.work is not None:
            self.work.wait()
        _convert(self.wire, self.dst)


def _allreduce_range(arena: "GradArena", lo: int, hi: int, async_op: bool):
    """SUM over ranks of arena.flat[lo:hi] in the configured wire format; returns something with .wait() (or None)."""
    import torch.distributed as dist
    if hi <= lo:
        return None
    piece = arena.flat[lo:hi]
    if _GRAD_WIRE_DTYPE == torch.float32:
        return dist.all_reduce(piece, async_op=True) if async_op else dist.all_reduce(piece)
    if getattr(arena, "wire", None) is None:
        arena.wire = torch.empty(arena.flat.numel(), dtype=torch.bfloat16, device=arena.flat.device)
    wire = _convert(piece, arena.wire[lo:hi])
    if async_op:
        return _WireWork(dist.all_reduce(wire, async_op=True), wire, piece)
    dist.all_reduce(wire)
    _convert(wire, piece)
    return None


def allreduce_arena(arena: GradArena) -> None:
    """The single gradient collective of a data-parallel step: SUM over ranks of the flat arena (RCCL over xGMI on
    MI355X; gloo in the CPU tests).  The loss gradient is pre-scaled by 1/world in train_step, so SUM == DDP's mean."""
    if collectives_on():
        _allreduce_range(arena, 0, arena.flat.numel(), False)


def allreduce_arena_early(arena: GradArena):
    """Start the all-reduce of the early-final range `flat[split:]` without blocking the launching stream (the collective
    runs on RCCL's own stream behind everything queued so far); returns the work handle (None for a single process)."""
    if collectives_on() and arena.split < arena.flat.numel():
        return _allreduce_range(arena, arena.split, arena.flat.numel(), True)
    return None


def allreduce_arena_late(arena: GradArena, early_work) -> None:
    """All-reduce the late range `flat[:split]` and join the early collective: afterwards the whole arena is reduced."""
    if collectives_on():
        if early_work is None:
            _allreduce_range(arena, 0, arena.flat.numel(), False)
            return
        _allreduce_range(arena, 0, arena.split, False)
        early_work.wait()


def _syncbn_shape_exchange(m, dev, shape_key):
    """SyncBatchNorm combines the ranks' moments assuming every rank holds the same number of samples per layer (bn_act; torch's
    SyncBatchNorm gathers per-rank counts instead, uneven last batches need drop_last=True here).  The check is collective-
    SYMMETRIC and never blocks the host: EVERY eager forward of EVERY rank gathers (B, H, W) with one tiny collective at the same
    point of the step (a rank that decided from its own shape history whether to take part - round 4 - could leave the others
    alone in the collective); the comparison stays on the device, a mismatch (a) turns the step's logits into NaN (a ReLU would
    swallow a NaN planted earlier), so its loss and gradients are visibly invalid, and (b) sets a sticky flag that travels to pinned host memory
    asynchronously: the next eager forward that finds the copy complete raises CavpError.  Captured steps replay the shape their
    eager warm-up pass was checked with.  Returns the 0-dim poison tensor (0.0 or NaN)."""
    st = m.__dict__.setdefault("_syncbn_check", {})
    if "event" in st and st["event"].query():
        if float(st["host"][0]) != 0.0:
            raise CavpError("SyncBatchNorm on the MI355X path needs the same batch and image size on every rank (a step with "
                            f"unequal shapes ran: its results are NaN; this rank last ran {st.get('last')}); use drop_last=True")
    tags = st.setdefault("tags", {})
    if shape_key not in tags:   # one small upload per NEW shape
        tags[shape_key] = torch.tensor([float(v) for v in shape_key], dtype=torch.float32, device=dev).reshape(3, 1)
    if "bad" not in st:
        st["bad"] = torch.zeros((1,), dtype=torch.float32, device=dev)
        st["host"] = torch.zeros((1,), dtype=torch.float32).pin_memory()
    got = gather_bn_moments(tags[shape_key])                      # [world, 3, 1]
    mism = (got != got[0:1]).any().to(torch.float32).reshape(1)   # device-side compare, no host read
    torch.maximum(st["bad"], mism, out=st["bad"])
    st["host"].copy_(st["bad"], non_blocking=True)
    st["event"] = torch.cuda.Event()
    st["event"].record(torch.cuda.current_stream())
    st["last"] = shape_key
    return torch.where(mism > 0, torch.full_like(mism, float("nan")), torch.zeros_like(mism)).reshape(())


def gather_bn_moments(local: torch.Tensor) -> torch.Tensor:
    """SyncBatchNorm forward exchange: every rank's per-channel (mean, M2) [C, 2] -> [world, C, 2] on every rank, ONE
    collective per layer.  RCCL: all-gather.  Other backends (gloo in the tests, which has no device all-gather): the same
    result as an all-reduce of a buffer that is zero outside this rank's slot."""
    import torch.distributed as dist
    world = dist.get_world_size()
    if dist.get_backend() == "nccl":
        out = torch.empty((world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous())
        return out
    out = torch.zeros((world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
    out[dist.get_rank()].copy_(local)
    dist.all_reduce(out)
    return out


# False (tests / A-B only): GELU as a separate pass with the pre-activation stored, and the duplicated token tensors copied
_FUSE_TOKEN_PATH = True
# False (tests / A-B only): the cross-modal attention as written in the reference - q GEMM, gate kernel, proj GEMM - instead of
# the one-key collapse (csrc/attn_rank1.hip)
_RANK1_ATTN = True
_SIDE_STREAM = True      # False (tests / A-B only): the audio encoder on the main stream
# Weight gradients are not consumed inside the backward: TrainPass collects them and issues up to 16 per launch
# (cavp_conv2d_wgrad_group).  False (tests / A-B only): one launch (+ one slab reduce) per layer, where the layer's backward runs.
_GROUP_WGRAD = True
_BRANCH_STREAM = True    # False (tests / A-B only): the down-sample branch of a bottleneck on the main stream (rounds 1-4)
_SIDE_PACKS = True       # False (A/B only): the audio encoder's weight re-packs on the main stream with all the others (rounds 1-4)
_FUSE_BN_BWD = True      # False (tests / A-B only): BatchNorm backward always as reduce launch + apply launch (rounds 1-4)
# The BatchNorm apply passes of launches with few tiles combine the per-tile statistics / partial sums themselves (one launch instead
# of combine + apply, bit-identical).  False (tests / A-B only): always the two launches.  The two tile limits are where the one
# launch won per launch on MI355X (profiles/bn_combine_in_apply.md): the backward up to 196 tiles; the forward, whose combine is a
# chain of divisions every workgroup repeats, only for the single-tile launch of the ASPP pooled branch.  The library declines
# above its own limit (train_ops.BN_FUSED_TILES) whatever is passed down.
_BN_COMBINE_IN_APPLY = True
_BN_COMBINE_FWD_TILES = 1
_BN_COMBINE_BWD_TILES = 196
_BN_BWD_READ_Y = False   # True (tests / A-B only): the BatchNorm backward always re-reads y instead of re-deriving the mask from z
# False (tests / A-B only): the ResNet-18 audio stem of the training pass as the two launches the fused one replaces (conv_smallcin_kxk,
# then col_tile_stats over the map it wrote)
_FUSE_AUDIO_STEM = True
_FUSE_STEM_POOL = True   # False (tests / A-B only): stem bn1 + ReLU and the max pool as two launches with the activation in memory (rounds 1-5)


def bump_counters(model, counters) -> None:
    """BatchNorm's num_batches_tracked += 1 for every layer that tracked statistics this step: ONE cavp_i64_add_table launch over a
    device table of the counters' addresses (cached on the model per counter set; the buffers keep their addresses)."""
    if not counters:
        return
    if counters[0].device.type != "cuda" or any(c.dtype != torch.int64 or c.numel() != 1 for c in counters):
        torch._foreach_add_(counters, 1)
        return
    key = tuple(c.data_ptr() for c in counters)
    cache = model.__dict__.setdefault("_cavp_nbt_tables", {})
    tab = cache.get(key)
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            torch._foreach_add_(counters, 1)   # (first sight of this counter set inside a capture: no host -> device copy here)
            return
        tab = torch.tensor(key, dtype=torch.int64).to(counters[0].device)
        cache[key] = tab
    T.i64_add_table(tab, 1)


class TrainPass:
    def __init__(self, model, dtype: torch.dtype, arena: Optional[GradArena] = None):
        self.m = model
        self.dt = dtype
        self.arena = arena
        self.touched = set()
        self.tape: List[Callable[[], None]] = []
        self.grads: Dict[int, torch.Tensor] = {}
        self.P: Dict[str, _P] = {}
        self._pack_jobs = []
        self._nbt = []   # BatchNorm num_batches_tracked counters bumped once, together, at the end of the forward
        self.on_early_final: Optional[Callable[[], None]] = None   # called in backward once head / attention / audio grads are final
        self.dev = next(model.parameters()).device
        self.named: Dict[str, V] = {}   # debug taps (activations + their gradients after backward)
        self.syncbn_poison: Optional[torch.Tensor] = None   # 0-dim 0.0 / NaN from _syncbn_shape_exchange, added to the logits
        # side section (the audio encoder): tape range run on a second stream, concurrently with the visual backbone
        self.side_range: Optional[tuple] = None
        self._side_done = None
        self._slot = 0
        self._zpools: Dict[int, list] = {}
        self._wg_jobs: list = []       # deferred weight gradients (main stream only), see wgrad() / flush_wgrads()
        self._wg_dst: set = set()
        self._wg_src: set = set()      # storages of their dy operands (see _pinned)
        self._wg_after: list = []      # callbacks run right behind the next grouped launch (defer_wgrad)

    # ---- parameter helpers -----------------------------------------------------------------------------------
    def pack(self, key: str, mod, need_dgrad: bool = True, raw: bool = False, pad_cout_to: int = 0) -> _P:
        p = _P()
        p.weight, p.bias = mod.weight, getattr(mod, "bias", None)
        p.real_weight = p.real_bias = None
        p.real_cout = 0
        if isinstance(mod, nn.Linear):
            p.kh = p.kw = 1
            p.stride, p.pad, p.dil = 1, 0, 1
            p.cout, p.cin = mod.out_features, mod.in_features
        else:
            p.kh, p.kw = mod.kernel_size
            p.stride, p.pad, p.dil = mod.stride[0], mod.padding[0], mod.dilation[0]
            p.cout, p.cin = mod.out_channels, mod.in_channels
        if pad_cout_to and p.cout % pad_cout_to:
            # Output channels that are not a multiple of the 16-byte vector (the classifier: C = 2, 22, 24, 71 ...):
            # run the layer on zero-padded weights so every kernel stays vectorised; the padding rows of the
            # gradient are dropped in `finish_padded`.
            cp = (p.cout + pad_cout_to - 1) // pad_cout_to * pad_cout_to
            wpad = torch.zeros((cp,) + tuple(mod.weight.shape[1:]), dtype=torch.float32, device=self.dev)
            ops.cast(mod.weight.detach().contiguous().view(-1), wpad[:p.cout].view(-1))
            p.real_weight, p.real_cout, p.weight = mod.weight, p.cout, wpad
            if p.bias is not None:
                bpad = torch.zeros(cp, dtype=torch.float32, device=self.dev)
                ops.cast(p.bias.detach().contiguous(), bpad[:p.cout])
                p.real_bias, p.bias = p.bias, bpad
            p.cout = cp
        # the re-packs themselves are deferred to flush_packs(): one multi-tensor launch instead of two per layer
        if raw:
            p.w, p.wT = p.weight.detach(), None
        else:
            p.w = torch.empty((p.cout, p.kh, p.kw, p.cin), dtype=self.dt, device=self.dev)
            p.wT = torch.empty((p.cin, p.kh, p.kw, p.cout), dtype=self.dt, device=self.dev) if need_dgrad else None
            self._pack_jobs.append((p.weight, p.w, p.wT))
        self.P[key] = p
        return p

    def flush_packs(self, keep_from: Optional[int] = None) -> list:
        """Issue the deferred re-packs; keep_from: the jobs from that index on are NOT issued but returned (the audio encoder's weights -
        two thirds of the bytes - are re-packed by the side stream that uses them, off the main stream's critical path)."""
        jobs, self._pack_jobs = self._pack_jobs, []
        held = []
        if keep_from is not None:
            jobs, held = jobs[:keep_from], jobs[keep_from:]
        T.pack_weights_multi(jobs, self.dt)
        return held

    def finish_padded(self) -> None:
        self.flush_wgrads()
        for p in self.P.values():
            if p.real_weight is None:
                continue
            for padded, real in ((p.weight, p.real_weight), (p.bias, p.real_bias)):
                if real is None:
                    continue
                g = self.grads.pop(id(padded), None)
                if g is None:
                    continue
                g = g[:p.real_cout]
                if self.arena is not None and id(real) in self.arena.views:
                    dst = self.arena.views[id(real)]
                    ops.cast(g.contiguous().view(-1), dst.view(-1))
                    g = dst
                self.grads[id(real)] = g
                self.touched.add(id(real))

    def add_grad(self, param: torch.Tensor, g: torch.Tensor) -> None:
        k = id(param)
        if k in self.grads or (self.arena is not None and k in self.arena.views):
            buf = self.grad_buffer(param)
            if g.numel() % 4 == 0:
                T.add(buf, g.reshape(buf.shape).contiguous(), buf)
            else:
                buf.add_(g.reshape(buf.shape))   # odd-sized vectors (never on the CAVP path; kept for safety)
        else:
            self.grads[k] = g.reshape(param.shape)
        self.touched.add(k)

    def grad_buffer(self, param: torch.Tensor, _overwrite: bool = False) -> torch.Tensor:
        """f32 zero-initialised gradient accumulator in the parameter's own layout (created on first use)."""
        k = id(param)
        self.touched.add(k)
        if k not in self.grads:
            if self.arena is not None and k in self.arena.views:
                self.grads[k] = self.arena.views[k]       # zeroed once per step by GradArena.zero() ...
                if k in self.arena.no_zero and not _overwrite:
                    T.zero_(self.grads[k])                # ... unless it is an overwrite-on-first-touch weight reached another way
            else:
                self.grads[k] = T.zeros(param.shape, torch.float32, self.dev)
        return self.grads[k]

    def empty(self, shape, dtype=None) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype or self.dt, device=self.dev)

    def zeros_f32(self, *shape) -> torch.Tensor:
        """Zero-initialised f32 scratch.  Small requests (BN statistics, bias / affine gradients: ~250 per step) are
        carved out of one pre-zeroed pool = one memset per step instead of one fill launch each."""
        n = 1
        for d in shape:
            n *= d
        if n > (1 << 16):
            return T.zeros(shape, torch.float32, self.dev)
        st = self._zpools.setdefault(self._slot, [None, 0])   # one pool per stream slot: a pool's fill is ordered on ITS stream only
        if st[0] is None or st[1] + n + 4 > st[0].numel():
            st[0] = T.zeros((1 << 21 if self._slot == 0 else 1 << 18,), torch.float32, self.dev)
            st[1] = 0
        t = st[0][st[1]:st[1] + n].view(shape)
        st[1] += (n + 3) // 4 * 4     # keep every carve 16-byte aligned
        return t

    # ---- gradient accumulation -------------------------------------------------------------------------------
    def acc(self, x: V, compute: Callable[[torch.Tensor, Optional[torch.Tensor]], None], bnb_token=None) -> None:
        """Run compute(out, residual) so that x.g += result (residual-add fused in the producing kernel).
        bnb_token: the caller is a conv whose data gradient can carry the BatchNorm-backward statistics of x (compute accepts
        bnb=...); used when this conv claimed x in the forward, i.e. when this contribution completes x.g."""
        if not x.needs_grad:
            return
        if x.parent is not None:
            raise CavpError("accumulating into a slice is not supported")
        if bnb_token is not None and x.bnb is not None and x.bnb_claim is bnb_token and x.grad_mul is None:
            if x.g is None:
                g, r = self.empty(x.t.shape, x.t.dtype), None
            elif self._pinned(x.g):
                g, r = self.empty(x.t.shape, x.t.dtype), x.g
            else:
                g, r = x.g, x.g
            part = compute(g, r, bnb=x.bnb)   # (partials, tiles), or None: this launch could not carry them (g is the plain gradient)
            x.set_g(g)
            x.bnb_part = part
            return
        if x.grad_mul is not None:
            # the single consumer of a fused-GELU hidden activation: d(pre) = d(hidden) * gelu'(pre) inside its epilogue
            if x.g is not None:
                raise CavpError("a fused-GELU activation takes its gradient from exactly one producer")
            g = self.empty(x.t.shape, x.t.dtype)
            compute(g, None, x.grad_mul)
            x.set_g(g)
            x.g_premul = True
            return
        if x.g is None:
            g = self.empty(x.t.shape, x.t.dtype)
            compute(g, None)
            x.set_g(g)
        elif self._pinned(x.g):   # a pending weight gradient still reads x.g (see wgrad()): accumulate out of place
            g = self.empty(x.t.shape, x.t.dtype)
            compute(g, x.g)
            x.set_g(g)
        else:
            compute(x.g, x.g)
            x.g_scaled = None
            x.bnb_part = None

    def _use(self, x: Optional[V]) -> None:
        """A non-conv op consumes x: if it is the FIRST consumer of a BatchNorm output, no conv completes that gradient.  EVERY tape
        op that takes a V calls this (or, conv: makes the claim itself) before it registers its backward."""
        if x is not None and x.bnb is not None and x.bnb_claim is None:
            x.bnb_claim = False

    def acc_add(self, x: V, g: torch.Tensor) -> None:
        if not x.needs_grad:
            return
        if x.parent is not None:
            raise CavpError("accumulating into a slice is not supported")
        if x.g is None:
            x.set_g(g if g.is_contiguous() else self._dense_copy(g))
        else:
            gg = g if g.is_contiguous() else self._dense_copy(g)
            if self._pinned(x.g):
                out = self.empty(x.g.shape, x.g.dtype)
                T.add(x.g, gg, out)
                x.set_g(out)
            else:
                T.add(x.g, gg, x.g)
                x.g_scaled = None
                x.bnb_part = None

    def _pinned(self, t: torch.Tensor) -> bool:
        """True while a deferred weight gradient reads t's storage: a conv with a fused residual hands its output gradient to
        the residual branch WITHOUT a copy (acc_add: x.g = g), so a later in-place accumulation into that branch's gradient
        would change the dy of the pending job.  The accumulation then goes into a fresh tensor (same traffic, no extra pass)."""
        if not self._wg_src:
            return False
        return t.untyped_storage().data_ptr() in self._wg_src

    def _dense_copy(self, g: torch.Tensor) -> torch.Tensor:
        out = self.empty(g.shape, g.dtype)
        T.scale_shift_act(g, None, None, out, ACT_NONE)
        return out

    # ---- ops -------------------------------------------------------------------------------------------------
    def conv(self, x: V, key: str, *, act: int = ACT_NONE, residual: Optional[V] = None, nbias: Optional[V] = None,
             out: Optional[V] = None, stats: bool = False, residual_periodic: bool = False) -> V:
        """y = act(conv(x) + nbias[n] + bias + residual); fused epilogue forward, tape entry for backward.
        stats=True or the BatchNorm module the conv feeds: ask the epilogue for the per-tile batch statistics (a module in eval
        mode normalises with its running statistics: nothing is collected).
        act=ACT_GELU (timm Mlp's fc1, attn.py:136-150): y = gelu(t) and gelu'(t) are both written by the epilogue; the
        pre-activation never reaches HBM and the backward multiplier is applied inside the GEMM that produces dy.
        residual_periodic: `residual` holds the first 1/k of the batch and is added to every k-th part (the un-duplicated half
        of forward_train's torch.cat((x, x.clone())), cavp_model.py:181); its gradient is the sum over the parts."""
        p = self.P[key]
        x4 = _as4(x.t)
        n, h, w, _ = x4.shape
        bnb_tok = None
        if x.bnb is not None and x.bnb_claim is None:
            # first consumer (forward order) of a BatchNorm + ReLU output = the LAST contributor to its gradient in the backward
            x.bnb_claim = bnb_tok = object() if (_FUSE_BN_BWD and x.parent is None and x.needs_grad and x.t.dim() == 4) else False
        self._use(residual)
        ho = (h + 2 * p.pad - p.dil * (p.kh - 1) - 1) // p.stride + 1
        wo = (w + 2 * p.pad - p.dil * (p.kw - 1) - 1) // p.stride + 1
        if out is None:
            out = V(self.empty(x.t.shape[:-1] + (p.cout,)) if x.t.dim() != 4 else self.empty((n, ho, wo, p.cout)))
        bias = p.bias.detach() if p.bias is not None else None
        bn_mod = stats if isinstance(stats, nn.modules.batchnorm._BatchNorm) else None
        if bn_mod is not None and (not bn_mod.training) and bn_mod.running_mean is not None:
            stats = False   # frozen statistics (eval-mode module): nobody reads batch statistics
        fuse = bool(stats) and bias is None and nbias is None and residual is None and act == ACT_NONE and out.parent is None
        deriv = self.empty(out.t.shape, out.t.dtype) if act == ACT_GELU else None
        res_rows = 0
        if residual_periodic:
            res_rows = residual.t.numel() // residual.t.shape[-1]
            if (out.t.numel() // out.t.shape[-1]) % res_rows or res_rows % 256:
                raise CavpError("periodic residual: its rows must divide the output's and be a multiple of 256")
        r = ops.conv2d(x4, p.w, _as4(out.t), kh=p.kh, kw=p.kw, stride=p.stride, pad=p.pad, dil=p.dil, shift=bias,
                       nbias=nbias.t if nbias is not None else None,
                       residual=_as4(residual.t) if residual is not None else None, act=act, want_tile_stats=fuse,
                       res_rows=res_rows, aux=_as4(deriv) if deriv is not None else None, aux_mode=1 if deriv is not None else 0)
        if fuse:
            out.tile_stats = r[1]
        y = out
        if deriv is not None:
            y.grad_mul = deriv

        def bwd():
            dy = y.g
            if dy is None:
                return
            if act in (ACT_RELU, ACT_LEAKY):
                g = self.empty(y.t.shape, y.t.dtype)
                T.act_bwd(dy, y.t, g, act)
            elif act == ACT_GELU:
                if not y.g_premul:
                    raise CavpError("fused GELU: the gradient must come from a data-gradient GEMM (TrainPass.acc)")
                g = dy   # already d(hidden) * gelu'(pre)
            else:
                g = dy
            if residual is not None:
                if residual_periodic:   # gradient of the shared residual = sum over the batch parts
                    rr = residual.t.numel() // residual.t.shape[-1]
                    g2 = g.reshape(-1, g.shape[-1])
                    parts = [g2[i:i + rr] for i in range(0, g2.shape[0], rr)]
                    acc_g = self.empty(residual.t.shape, residual.t.dtype)
                    T.add(parts[0], parts[1], acc_g.view(rr, -1))
                    for extra in parts[2:]:
                        T.add(acc_g.view(rr, -1), extra, acc_g.view(rr, -1))
                    self.acc_add(residual, acc_g)
                else:
                    self.acc_add(residual, g)
            if nbias is not None:
                nb = self.zeros_f32(*nbias.t.shape)
                T.colsum_groups(_as4(g), nb)      # one launch for all images (was one column-sum launch per image)
                self.acc_add(nbias, nb)
            self.wgrad(p, x4, _as4(g))      # (+ the bias gradient: column sums of g taken inside the same kernel)
            if x.needs_grad:
                def dg(o, r, mul=None, bnb=None):
                    return T.conv2d_dgrad(_as4(g), p.wT, _as4(o), kh=p.kh, kw=p.kw, stride=p.stride, pad=p.pad, dil=p.dil,
                                          residual=_as4(r) if r is not None else None, mul=_as4(mul) if mul is not None else None,
                                          bnb=bnb)
                self.acc(x, dg, bnb_token=bnb_tok)
        self.tape.append(bwd)
        return y

    def wgrad(self, p: _P, x4: torch.Tensor, g4: torch.Tensor) -> None:
        db = self.grad_buffer(p.bias) if p.bias is not None else None
        k = id(p.weight)
        # first contribution of the step to a weight the arena does not clear: beta = 0 (the view may hold last step's gradient)
        ow = self.arena is not None and k in self.arena.no_zero and k not in self.grads and k not in self.touched
        dw = self.grad_buffer(p.weight, _overwrite=ow)
        if p.kh * p.kw == 1:   # OHWI == OIHW for 1x1 / linear: straight into the gradient
            job = dict(x=x4, dy=g4, dw=dw.view(p.cout, 1, 1, p.cin), kh=1, kw=1, stride=p.stride, pad=p.pad, dil=p.dil, dbias=db,
                       overwrite=ow)
        else:   # k x k: the kernel writes the torch-layout gradient directly (no OHWI temporary + unpack pass)
            job = dict(x=x4, dy=g4, dw=dw, kh=p.kh, kw=p.kw, stride=p.stride, pad=p.pad, dil=p.dil, dbias=db, dw_oihw=True,
                       overwrite=ow)
        self.defer_wgrad(job)

    def defer_wgrad(self, job: dict, after: Optional[Callable[[], None]] = None) -> None:
        """Queue one weight-gradient job (the arguments of train_ops.conv2d_wgrad as a dict).  Nothing in the backward chain
        reads a weight gradient, so the jobs wait (holding x and dy alive) until 16 are pending or a flush point is reached, and
        go out as ONE launch (cavp_conv2d_wgrad_group).  `after` runs right behind that launch (e.g. the un-permutation of a
        gradient the GEMM produced in another layout)."""
        x4, g4, dw, db = job["x"], job["dy"], job["dw"], job.get("dbias")
        if not _GROUP_WGRAD or self._slot != 0 or x4.dtype != self.dt:
            j = dict(job)
            T.conv2d_wgrad(j.pop("x"), j.pop("dy"), j.pop("dw"), **j)   # (the side stream keeps its per-layer launches)
            if after is not None:
                after()
            return
        # a second contribution to a destination that is already pending would race inside the launch: flush first
        dst = {dw.data_ptr()} | ({db.data_ptr()} if db is not None else set())
        if dst & self._wg_dst:
            self.flush_wgrads()
        self._wg_jobs.append(job)
        self._wg_dst |= dst
        self._wg_src.add(g4.untyped_storage().data_ptr())
        if after is not None:
            self._wg_after.append(after)
        if len(self._wg_jobs) >= 16:
            self.flush_wgrads()

    def flush_wgrads(self) -> None:
        """Issue the pending weight gradients as one grouped launch on the current stream (before anything reads a parameter gradient or
        overwrites an operand: finish_padded, the early / late gradient collectives, the end of the backward; also a full group and a
        second contribution to a pending destination).  (Rounds 3-5 could put the groups on a stream of their own: measured slower
        both times - a resident weight-gradient workgroup owns its CU's LDS, the two streams serialise at workgroup granularity
        (profiles/r05_notes.md 4d) - and removed in round 6.)"""
        if self._wg_jobs:
            jobs, self._wg_jobs, self._wg_dst = self._wg_jobs, [], set()
            after, self._wg_after = self._wg_after, []
            self._wg_src = set()
            T.conv2d_wgrad_group(jobs)
            for fn in after:
                fn()

    def conv_smallcin(self, x_nchw: torch.Tensor, key: str, stride: int, act: int) -> V:
        """First stem conv (raw, BN follows) / first VGG conv (bias + ReLU fused).  Input needs no gradient."""
        p = self.P[key]
        n, _, h, w = x_nchw.shape
        y = V(self.empty((n, (h - 1) // stride + 1, (w - 1) // stride + 1, p.cout)))
        bias = p.bias.detach() if p.bias is not None else None
        ops.conv3x3_smallcin_nchw(x_nchw, p.w, y.t, stride=stride, scale=None, shift=bias, act=act)

        def bwd():
            dy = y.g
            if dy is None:
                return
            g = dy
            if act in (ACT_RELU, ACT_LEAKY):
                g = self.empty(y.t.shape, y.t.dtype)
                T.act_bwd(dy, y.t, g, act)
            if p.bias is not None:
                T.colsum(g, self.grad_buffer(p.bias))
            T.smallcin_wgrad(x_nchw, g, self.grad_buffer(p.weight), stride)
        self.tape.append(bwd)
        return y

    def audio_stem(self, x_nchw: torch.Tensor, key: str) -> V:
        """conv1 of the ResNet-18 audio encoder (7 x 7, stride 2, pad 3, no bias; f32 NCHW input with 1 or 2 channels, no input
        gradient), raw, with the BatchNorm tile statistics of its output from the same launch (train_ops.audio_stem_train)."""
        p = self.P[key]
        n, _, h, w = x_nchw.shape
        y = V(self.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, p.cout)))
        # (a bn1 in eval() normalises with its running statistics and never reads this table: the launch still takes it - a few
        # microseconds of reductions - so that there is one stem launch, not a second variant without them)
        y.tile_stats = T.audio_stem_train(x_nchw, p.w, y.t, fused=_FUSE_AUDIO_STEM)

        def bwd():
            if y.g is None:
                return
            g = y.g if y.g.is_contiguous() else self._dense_copy(y.g)
            T.conv_smallcin_kxk_wgrad(x_nchw, g, self.grad_buffer(p.weight), p.kh, p.stride, p.pad)
        self.tape.append(bwd)
        return y

    def bn_act(self, z: V, bn, act: int, residual: Optional[V] = None, out: Optional[V] = None,
               pool: Optional[Tuple[int, int, int]] = None) -> V:
        """y = act(BN_train(z) + residual); `out` may be a channel slice of a concat buffer.
        pool = (k, stride, pad): y = max_pool(act(BN_train(z))) in ONE pass over z (the stem: bn1 -> relu -> maxpool, resnet.py:187-190) -
        the un-pooled activation is never stored; the backward routes the pooled gradient through the arg-max first and then is the
        ordinary BatchNorm + activation backward with the mask re-derived from z."""
        c = bn.num_features
        rows = z.t.numel() // z.t.shape[-1]
        scale, shift, mean, rstd = (self.empty((c,), torch.float32) for _ in range(4))
        track = bn.track_running_stats and bn.running_mean is not None
        mom = bn.momentum if bn.momentum is not None else 0.1
        sync = isinstance(bn, nn.SyncBatchNorm) and collectives_on()   # (a forced single-rank group runs the collectives too)
        frozen = (not bn.training) and bn.running_mean is not None   # torch: eval-mode BatchNorm normalises with the running statistics
        fused_tiles = None
        if frozen:
            # fine-tuning with frozen statistics: y = gamma (z - running_mean) rstd + beta, no update of the running buffers;
            # backward dz = gamma rstd g, dgamma = sum g zhat, dbeta = sum g (no batch-mean terms)
            from . import ops as O
            track, count = False, rows
            O.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, scale, shift)
            one, zero = self.empty((c,), torch.float32).fill_(1.0), self.zeros_f32(c)
            O.bn_fold(one, zero, bn.running_mean, bn.running_var, bn.eps, rstd, zero.clone())
            mean = bn.running_mean
        elif not sync:
            # per-tile (mean, M2) - out of the producing conv's epilogue, or (split-K convs, the small-Cin stem, channel slices of a
            # concat buffer) from one pass over z - combined by Chan's formula: cancellation-free, also for the M = B rows of the
            # ASPP pooled branch
            ts, tiles, rpt = z.tile_stats if z.tile_stats is not None else T.col_tile_stats(z.t)
            count = rows
            if _BN_COMBINE_IN_APPLY and pool is None and tiles <= _BN_COMBINE_FWD_TILES:
                # few tiles: the apply launch below combines them for its own channel slices
                fused_tiles = (ts, tiles, rpt, bn.weight.detach(), bn.bias.detach(), bn.eps, mom,
                               bn.running_mean if track else None, bn.running_var if track else None, mean, rstd)
            else:
                T.bn_finalize_tiles(ts, tiles, rpt, rows, bn.weight.detach(), bn.bias.detach(), bn.eps, mom,
                                    bn.running_mean if track else None, bn.running_var if track else None, scale, shift,
                                    mean, rstd)
        else:
            # SyncBatchNorm (main_vpo_mono.py:130): this rank's (mean, M2) -> ONE all-gather -> Chan combine over the ranks (the
            # same kernel that combines tiles; every rank holds `rows` samples).  Round 1 issued three all-reduces per layer.
            world = dist_world()
            ts, tiles, rpt = z.tile_stats if z.tile_stats is not None else T.col_tile_stats(z.t)
            local = self.empty((c, 2), torch.float32)
            T.bn_tiles_to_moments(ts, tiles, rpt, rows, local)
            gathered = gather_bn_moments(local)
            count = rows * world
            T.bn_finalize_tiles(gathered, world, rows, count, bn.weight.detach(), bn.bias.detach(), bn.eps, mom,
                                bn.running_mean if track else None, bn.running_var if track else None, scale, shift,
                                mean, rstd)
        if track and bn.num_batches_tracked is not None:
            self._nbt.append(bn.num_batches_tracked)
        am = None
        if pool is not None:
            if residual is not None or out is not None or z.t.dim() != 4:
                raise ValueError("bn_act(pool=...): plain NHWC BatchNorm + activation only")
            pk, ps, pp = pool
            n_, h_, w_, c_ = z.t.shape
            y = V(self.empty((n_, (h_ + 2 * pp - pk) // ps + 1, (w_ + 2 * pp - pk) // ps + 1, c_), z.t.dtype))
            am = torch.empty(y.t.shape, dtype=torch.uint8, device=self.dev)
            ops.maxpool(z.t, y.t, pk, ps, pp, argmax=am, scale=scale, shift=shift, act=act)
        else:
            y = out if out is not None else V(self.empty(z.t.shape, z.t.dtype))
            if fused_tiles is not None:
                T.scale_shift_act(z.t, scale, shift, y.t, act, residual=residual.t if residual is not None else None,
                                  bn_tiles=fused_tiles)
            else:
                T.scale_shift_act(z.t, scale, shift, y.t, act, residual=residual.t if residual is not None else None)

        self._use(residual)
        # (ReLU only: its mask is idempotent, so the fallback - a later contribution drops the partial sums and the separate reduce / apply
        # passes mask the already-masked sum once more - stays exact; a LeakyReLU slope would be applied twice.  No LeakyReLU layer
        # of the CAVP graph qualified anyway: ASPP's outputs are concat slices.)
        if _FUSE_BN_BWD and not sync and not frozen and act == ACT_RELU and y.parent is None and z.t.dim() == 4 and pool is None:
            y.bnb = dict(z=z.t, out=y.t if residual is not None else None, scale=scale, shift=shift, mean=mean, rstd=rstd, act=act)

        def bwd():
            dy = y.g
            if dy is None:
                return
            if pool is not None:   # pooled gradient -> gradient of the (never stored) activation, through the recorded arg-max
                dpool = dy if dy.is_contiguous() else self._dense_copy(dy)
                dy = self.empty(z.t.shape, z.t.dtype)
                T.maxpool_bwd(am, dpool, dy, *pool)
            direct = (not sync and id(bn.weight) not in self.grads and id(bn.bias) not in self.grads)
            if y.bnb_part is not None:
                # the launch that completed dy already applied the activation's derivative and summed g and g * zhat per tile:
                # sum over the tiles, then the apply pass on the masked gradient (no mask, no second output: dy IS the skip gradient)
                part, tiles = y.bnb_part
                dz = self.empty(z.t.shape, z.t.dtype)
                sums = (self.grad_buffer(bn.bias), self.grad_buffer(bn.weight)) if direct else self.zeros_f32(2, c)
                if _BN_COMBINE_IN_APPLY and tiles <= _BN_COMBINE_BWD_TILES:
                    # (`sums` is zero here on both paths: a gradient buffer on its first touch of the step, or fresh zeroed scratch)
                    T.bn_act_bwd_apply(dy, None, z.t, mean, rstd, bn.weight.detach(), sums[0], sums[1], ACT_NONE, dz,
                                       tile_partials=(part, tiles))
                else:
                    T.bn_bwd_sum_tiles(part, tiles, sums[0], sums[1])
                    T.bn_act_bwd_apply(dy, None, z.t, mean, rstd, bn.weight.detach(), sums[0], sums[1], ACT_NONE, dz)
                z.set_g(dz)
                if residual is not None and residual.needs_grad:
                    self.acc_add(residual, dy)
                if not direct:
                    self.add_grad(bn.bias, sums[0].clone())
                    self.add_grad(bn.weight, sums[1].clone())
                return
            if direct:
                # local BatchNorm: sum g -> dbeta and sum g*zhat -> dgamma ARE the affine gradients: reduce straight
                # into their (zeroed) gradient buffers and let the apply kernel read them from there
                sums = (self.grad_buffer(bn.bias), self.grad_buffer(bn.weight))
            else:
                sums = self.zeros_f32(2, c)
            # without a residual the activation mask follows from z and the folded (scale, shift): y is not re-read
            yb = y.t if ((residual is not None or _BN_BWD_READ_Y) and pool is None) else None
            T.bn_act_bwd_reduce(dy, yb, z.t, mean, rstd, act, sums[0], sums[1], fwd_scale=scale, fwd_shift=shift)
            local = sums
            if sync and not frozen:   # (frozen statistics: dz has no batch-mean terms, nothing to exchange)
                # SyncBatchNorm: dz uses the GLOBAL sums / count, the affine gradients stay the LOCAL sums (DDP
                # reduces them with every other parameter gradient) - same split as torch's SyncBatchNorm backward
                import torch.distributed as dist
                local = sums.clone()
                dist.all_reduce(sums)
                sums = sums * (float(rows) / float(count))
            if frozen:
                sums = self.zeros_f32(2, c)     # the batch-mean terms of dz vanish; `local` keeps the affine gradients
            dz = self.empty(z.t.shape, z.t.dtype)
            g_out = self.empty(z.t.shape, z.t.dtype) if (residual is not None and residual.needs_grad) else None
            T.bn_act_bwd_apply(dy, yb, z.t, mean, rstd, bn.weight.detach(), sums[0], sums[1], act, dz, g_out=g_out,
                               fwd_scale=scale, fwd_shift=shift)
            z.set_g(dz)
            if g_out is not None:
                self.acc_add(residual, g_out)
            if not direct:
                self.add_grad(bn.bias, local[0].clone())
                self.add_grad(bn.weight, local[1].clone())
        self.tape.append(bwd)
        return y

    def gelu(self, x: V) -> V:
        self._use(x)
        y = V(self.empty(x.t.shape, x.t.dtype))
        T.scale_shift_act(x.t, None, None, y.t, ACT_GELU)

        def bwd():
            if y.g is None:
                return
            def f(o, r):
                if r is None:
                    T.act_bwd(y.g, x.t, o, ACT_GELU)
                else:
                    tmp = self.empty(x.t.shape, x.t.dtype)
                    T.act_bwd(y.g, x.t, tmp, ACT_GELU)
                    T.add(r, tmp, o)
            self.acc(x, f)
        self.tape.append(bwd)
        return y

    def maxpool(self, x: V, k: int, stride: int, pad: int) -> V:
        self._use(x)
        n, h, w, c = x.t.shape
        y = V(self.empty((n, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1, c)))
        am = torch.empty(y.t.shape, dtype=torch.uint8, device=self.dev)
        ops.maxpool(x.t, y.t, k, stride, pad, argmax=am)

        def bwd():
            if y.g is None:
                return
            dx = self.empty(x.t.shape, x.t.dtype)
            T.maxpool_bwd(am, y.g if y.g.is_contiguous() else self._dense_copy(y.g), dx, k, stride, pad)
            self.acc_add(x, dx)
        self.tape.append(bwd)
        return y

    def gmp(self, x: V) -> V:
        """nn.AdaptiveMaxPool2d((1, 1)) with its winner recorded (the first maximum in scan order); the backward writes the whole map's
        gradient in one pass: the pooled gradient at the winner, 0 elsewhere."""
        self._use(x)
        n, h, w, c = x.t.shape
        y = V(self.empty((n, c), x.t.dtype))
        am = torch.empty((n, c), dtype=torch.int32, device=self.dev)
        ops.global_maxpool_arg(x.t, y.t, am)

        def bwd():
            if y.g is None:
                return
            dx = self.empty(x.t.shape, x.t.dtype)
            T.global_maxpool_bwd(am, y.g if y.g.is_contiguous() else self._dense_copy(y.g), dx)
            self.acc_add(x, dx)
        self.tape.append(bwd)
        return y

    def gap(self, x: V) -> V:
        self._use(x)
        n, h, w, c = x.t.shape
        y = V(self.empty((n, c), torch.float32))
        ops.global_avgpool(x.t, y.t)

        def bwd():
            if y.g is None:
                return
            if x.g is None:
                x.set_g(T.zeros(x.t.shape, x.t.dtype, self.dev))
            elif self._pinned(x.g):
                self.flush_wgrads()   # in-place update of a gradient a pending weight gradient reads
            T.bcast_add(x.g, y.g, 1.0 / (h * w))
            x.bnb_part = None   # (in-place accumulation)
        self.tape.append(bwd)
        return y

    def cast(self, x: V, dtype: torch.dtype) -> V:
        self._use(x)
        if x.t.dtype == dtype:
            return x
        y = V(ops.cast(x.t.contiguous(), self.empty(x.t.shape, dtype)))

        def bwd():
            if y.g is None:
                return
            g = ops.cast(y.g.contiguous(), self.empty(x.t.shape, x.t.dtype))
            self.acc_add(x, g)
        self.tape.append(bwd)
        return y

    def bilinear(self, x: V, out: V, align_corners: bool) -> V:
        self._use(x)
        ops.bilinear(x.t, out.t, align_corners)

        def bwd():
            if out.g is None:
                return
            dx = self.empty(x.t.shape, x.t.dtype)
            T.bilinear_bwd(out.g, dx, align_corners)
            self.acc_add(x, dx)
        self.tape.append(bwd)
        return out

    def layernorm(self, x: V, ln, _done: Optional[V] = None) -> V:
        """_done: the normalised tensor when a fused kernel already produced it (pvt_train: residual + DropPath + LayerNorm)."""
        self._use(x)
        y = _done if _done is not None else V(self.empty(x.t.shape, x.t.dtype))
        if _done is None:
            ops.layernorm(x.t, ln.weight.detach(), ln.bias.detach(), y.t, ln.eps)

        def bwd():
            if y.g is None:
                return
            if not x.needs_grad:
                dx = self.empty(x.t.shape, x.t.dtype)
                T.layernorm_bwd(y.g, x.t, ln.weight.detach(), dx, self.grad_buffer(ln.weight), self.grad_buffer(ln.bias), ln.eps)
                return
            # the residual stream usually delivered its gradient already: it is added inside the kernel (into a fresh tensor while
            # a deferred weight gradient still reads the old one, in place otherwise)
            have = x.g if (x.parent is None and x.g is not None and x.g.is_contiguous() and x.g.dtype == x.t.dtype
                           and x.g.shape == x.t.shape) else None
            dx = have if (have is not None and not self._pinned(have)) else self.empty(x.t.shape, x.t.dtype)
            # x = residual + DropPath(branch): the branch's gradient (factor * dx) leaves the same kernel as a second output
            # (this norm is the last contributor to x.g on a transformer block's residual stream; if it is not, the next
            # accumulation drops the copy and the residual's backward scales x.g itself)
            first = have is None and x.g is None
            sc = self.empty(x.t.shape, x.t.dtype) if (x.dp_scale is not None and x.parent is None and (have is not None or first)) else None
            T.layernorm_bwd(y.g, x.t, ln.weight.detach(), dx, self.grad_buffer(ln.weight), self.grad_buffer(ln.bias), ln.eps,
                            add=have, scaled=sc, row_scale=x.dp_scale if sc is not None else None)
            if have is None:
                self.acc_add(x, dx)
            elif dx is not have:
                x.set_g(dx)
            if sc is not None:
                x.g_scaled = sc
        self.tape.append(bwd)
        return y

    def attn_gate(self, q: V, k: V, v: V, heads: int, scale: float):
        """q may hold only the first 1/k of the batch (the query projection of the un-duplicated images): batch item b reads
        q[b % q_batch]; dq is then the sum over the k parts."""
        self._use(q)
        self._use(k)
        self._use(v)
        qb, t, c = q.t.shape
        b = k.t.shape[0]
        attn = V(self.empty((b, heads, t), torch.float32))
        o = V(self.empty((b, t, c), q.t.dtype))
        ops.attn_gate(q.t, k.t, v.t, o.t, attn.t, heads, scale)

        def bwd():
            if o.g is None and attn.g is None:
                return
            do = o.g if o.g is not None else torch.zeros_like(o.t)
            dq = self.empty(o.t.shape, q.t.dtype)
            dk, dv = self.zeros_f32(b, c), self.zeros_f32(b, c)
            T.attn_gate_bwd(do, q.t, k.t, v.t, attn.t, attn.g, dq, dk, dv, heads, scale)
            if qb != b:
                parts = [dq[i:i + qb] for i in range(0, b, qb)]
                dqs = self.empty(q.t.shape, q.t.dtype)
                T.add(parts[0], parts[1], dqs)
                for extra in parts[2:]:
                    T.add(dqs, extra, dqs)
                dq = dqs
            self.acc_add(q, dq)
            self.acc_add(k, dk if k.t.dtype == torch.float32 else ops.cast(dk, self.empty(dk.shape, k.t.dtype)))
            self.acc_add(v, dv if v.t.dtype == torch.float32 else ops.cast(dv, self.empty(dv.shape, v.t.dtype)))
        self.tape.append(bwd)
        return o, attn

    def attn_rank1(self, x: V, k: V, v: V, attn_mod) -> tuple:
        """Attention with one key / value token per batch item + output projection + residual, collapsed to rank-H operations
        (csrc/attn_rank1.hip; attn.py:73-106, 153-156): r1 = x + proj(sigmoid(scale q k^T) v) with q = attn.q(x).  x: [xb, T, C]
        (xb divides the batch of k / v: forward_train's duplicated images are read, never copied); returns (r1 [B, T, C], attn).
        The weights are read as f32 (no bf16 re-pack of attn.q / attn.proj); their gradients land in the flat arena."""
        self._use(x)
        self._use(k)
        self._use(v)
        heads, scale = attn_mod.num_heads, attn_mod.scale
        wq, wp, bp = attn_mod.q.weight.detach(), attn_mod.proj.weight.detach(), attn_mod.proj.bias
        xb, t, c = x.t.shape
        b = k.t.shape[0]
        u, pm = ops.attn1_prepare(wq, wp, k.t, v.t, heads, scale)
        attn = V(self.empty((b, heads, t), torch.float32))
        r1 = V(self.empty((b, t, c), x.t.dtype))
        ops.attn1_fwd(x.t, u, pm, bp.detach() if bp is not None else None, r1.t, attn.t)

        def bwd():
            if r1.g is None:
                return
            if attn.g is not None:
                raise CavpError("attn_rank1: a gradient through the attention map is not supported (attn_v is an output only)")
            dx = self.empty(x.t.shape, x.t.dtype)
            du, dp = T.attn1_bwd(r1.g, x.t, u, pm, dx, self.grad_buffer(bp) if bp is not None else None)
            dk, dv = T.attn1_finish(wq, wp, k.t, v.t, du, dp, self.grad_buffer(attn_mod.q.weight), self.grad_buffer(attn_mod.proj.weight),
                                    heads, scale)
            self.acc_add(x, dx)
            self.acc_add(k, dk if k.t.dtype == torch.float32 else ops.cast(dk, self.empty(dk.shape, k.t.dtype)))
            self.acc_add(v, dv if v.t.dtype == torch.float32 else ops.cast(dv, self.empty(dv.shape, v.t.dtype)))
        self.tape.append(bwd)
        return r1, attn

    def dup2(self, x: V) -> V:
        """torch.cat((x, x.clone()), 0) (cavp_model.py:181)."""
        self._use(x)
        n = x.t.shape[0]
        y = V(self.empty((2 * n,) + tuple(x.t.shape[1:]), x.t.dtype))
        ops.cast(x.t, y.t[:n])
        ops.cast(x.t, y.t[n:])

        def bwd():
            if y.g is None:
                return
            g = self.empty(x.t.shape, x.t.dtype)
            T.add(y.g[:n], y.g[n:], g)
            self.acc_add(x, g)
        self.tape.append(bwd)
        return y

    def gather_cat(self, x: V, idx: torch.Tensor) -> V:
        """torch.cat((x, x[idx])) over rows (forward_audio, cavp_model.py:171-173); backward: dx = g[:B] + scatter-add of
        g[B:] by idx, accumulated row by row with the add kernel (B rows of 304 values, once per step)."""
        self._use(x)
        n = x.t.shape[0]
        y = V(torch.cat((x.t, x.t.index_select(0, idx)), dim=0))
        rows = [int(i) for i in idx.tolist()]

        def bwd():
            if y.g is None:
                return
            g = y.g[:n].clone()
            for j, i in enumerate(rows):
                T.add(g[i], y.g[n + j].contiguous(), g[i])
            self.acc_add(x, g)
        self.tape.append(bwd)
        return y

    def flatten(self, x: V) -> V:
        """[B, H, W, C] -> [B, H*W*C] view (VGG NHWC flatten)."""
        self._use(x)
        y = V(x.t.reshape(x.t.shape[0], -1))
        shape = x.t.shape

        def bwd():
            if y.g is not None:
                self.acc_add(x, y.g.reshape(shape))
        self.tape.append(bwd)
        return y

    def reshape(self, x: V, shape) -> V:
        self._use(x)
        y = V(x.t.view(shape))
        old = x.t.shape

        def bwd():
            if y.g is not None:
                self.acc_add(x, y.g.view(old))
        self.tape.append(bwd)
        return y

    def grad_tap(self, x: V, fn: Callable[[torch.Tensor], Optional[bool]]) -> V:
        """Identity in the forward.  In the backward, once every consumer recorded after this call has contributed to x.g,
        fn(g) adds a further (typically sparse) gradient into `g` in place; it returns False when it had nothing to add.  Follows
        acc()'s rules: the add goes into a copy while a deferred weight gradient still reads x.g, and the by-products of the
        launch that wrote x.g (g_scaled, bnb_part) are dropped once x.g has changed."""
        self._use(x)
        if x.parent is not None:
            raise CavpError("a gradient tap on a slice is not supported")

        def bwd():
            if not x.needs_grad:
                return
            g = x.g
            if g is None:
                g = T.zeros(x.t.shape, x.t.dtype, self.dev)
            elif self._pinned(g) or not g.is_contiguous():
                g = self._dense_copy(g)
            wrote = fn(g) is not False
            if g is not x.g:
                if wrote:
                    x.set_g(g)
            elif wrote:
                x.g_scaled = None
                x.bnb_part = None
        self.tape.append(bwd)
        return x

    def mark_early_grads_final(self) -> None:
        """Tape marker: everything recorded AFTER this point in the forward (audio encoder, projector, cross attention,
        decoder head) has its parameter gradients complete when the backward reaches it."""
        def bwd():
            self.flush_wgrads()
            self.finish_padded()            # the zero-padded classifier's gradient rows -> its real .grad view
            if self.on_early_final is not None:
                self.join_side()            # the audio encoder's gradients are part of the early range
                self.on_early_final()
        self.tape.append(bwd)

    # ---- side section ------------------------------------------------------------------------------------------
    def side_stream(self):
        """Second stream for the side section, or None (CPU tensors, deterministic mode: its scratch is process-wide)."""
        if self.dev.type != "cuda" or not _SIDE_STREAM or _lib_load().cavp_get_deterministic():
            return None
        if getattr(self.m, "seg_model", "") == "PVT":
            return None   # measured: beside PVTv2's ~5000 small launches the second branch costs 3.6 % (51.05 -> 52.9 ms) instead of saving
        s = getattr(self.m, "_side_stream", None)
        if s is None or s.device != self.dev:
            s = torch.cuda.Stream(device=self.dev)
            self.m.__dict__["_side_stream"] = s
        return s

    def branch_stream(self):
        """Third stream: the down-sample branch of a layer's first bottleneck in the forward (None: CPU tensors, deterministic mode -
        process-wide scratch -, SyncBatchNorm with live collectives - their order across ranks must not depend on stream timing -, A/B switch)."""
        if self.dev.type != "cuda" or not _BRANCH_STREAM or _lib_load().cavp_get_deterministic() or collectives_on():
            return None
        s = getattr(self.m, "_branch_stream", None)
        if s is None or s.device != self.dev:
            s = torch.cuda.Stream(device=self.dev)
            self.m.__dict__["_branch_stream"] = s
        return s

    def join_side(self) -> None:
        """Make the current stream wait for the side section's backward (its parameter gradients are final after this)."""
        if self._side_done is not None:
            torch.cuda.current_stream().wait_event(self._side_done)
            self._side_done = None

    def backward(self) -> None:
        side = self.side_stream() if self.side_range is not None else None
        i0, i1 = self.side_range if side is not None else (-1, -1)
        i = len(self.tape) - 1
        while i >= 0:
            if i == i1 - 1:
                # fork: everything recorded after the side section (fusion, head) has been issued; its gradients feed both
                # the side section's backward and the rest of the main tape, which now run concurrently
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream())
                side.wait_event(ev)
                with torch.cuda.stream(side), ops.workspace_slot(1):
                    self._slot = 1
                    try:
                        for j in range(i1 - 1, i0 - 1, -1):
                            self.tape[j]()
                    finally:
                        self._slot = 0
                    self._side_done = torch.cuda.Event()
                    self._side_done.record(side)
                i = i0 - 1
                continue
            self.tape[i]()
            i -= 1
        self.flush_wgrads()
        self.join_side()
        self.tape = []


# ---------------------------------------------------------------------------------------------------------------
# the model graph in training mode
# ---------------------------------------------------------------------------------------------------------------
def _pack_head(tp: TrainPass, m) -> None:
    up = m.segment.upsample
    tp.pack("head0", up.last_conv[0])
    tp.pack("head1", up.last_conv[3])
    tp.pack("cls", up.classifier, pad_cout_to=8)


def _pack_audio18(tp: TrainPass, rn) -> None:
    tp.pack("a18.stem", rn.conv1, raw=True)   # f32 OIHW, as cavp_audio_stem_train reads it
    for li in range(4):
        for bi, blk in enumerate(getattr(rn, f"layer{li + 1}")):
            key = f"a18.l{li + 1}.{bi}"
            tp.pack(key + ".c1", blk.conv1)
            tp.pack(key + ".c2", blk.conv2)
            if blk.downsample is not None:
                tp.pack(key + ".ds", blk.downsample[0])
    tp.pack("a18.fc", rn.fc)


def _audio18_stage(tp: TrainPass, rn, audio: torch.Tensor) -> V:
    """The ResNet-18 audio encoder (audio_network.py:18-25; torchvision ResNet._forward_impl) on the tape: [N, in_plane, T, F] f32 ->
    features [N, latent], no activation behind fc.  BatchNorm as TrainPass.bn_act has it: batch statistics (running statistics and
    counters updated) for a module in training mode, frozen statistics with gradients for one in eval mode."""
    if audio.dim() != 4 or audio.shape[1] != rn.in_plane:
        raise CavpError(f"ResNet-18 audio encoder was built with in_plane={rn.in_plane}: expected [N, {rn.in_plane}, T, F] log-mel "
                        f"input, got {tuple(audio.shape)}")
    if audio.dtype != torch.float32:
        raise CavpError("audio must be float32 (it is converted on the fly by the stem kernel)")
    z = tp.audio_stem(audio, "a18.stem")
    x = tp.bn_act(z, rn.bn1, ACT_RELU, pool=(3, 2, 1))
    for li in range(4):
        for bi, blk in enumerate(getattr(rn, f"layer{li + 1}")):
            key = f"a18.l{li + 1}.{bi}"
            o = tp.bn_act(tp.conv(x, key + ".c1", stats=blk.bn1), blk.bn1, ACT_RELU)
            if blk.downsample is not None:
                res = tp.bn_act(tp.conv(x, key + ".ds", stats=blk.downsample[1]), blk.downsample[1], ACT_NONE)
            else:
                res = x
            x = tp.bn_act(tp.conv(o, key + ".c2", stats=blk.bn2), blk.bn2, ACT_RELU, residual=res)
        tp.named[f"a18.layer{li + 1}"] = x
    p = tp.gmp(x)
    tp.named["a18.pool"] = p
    return tp.conv(p, "a18.fc")


def _pack_audio(tp: TrainPass, m) -> None:
    from .cavp_model import ResNet18Audio
    if isinstance(m.audio_backbone.backbone, ResNet18Audio):
        return _pack_audio18(tp, m.audio_backbone.backbone)
    vgg = m.audio_backbone.backbone
    convs = [mm for mm in vgg.features if isinstance(mm, nn.Conv2d)]
    tp.pack("a.conv0", convs[0], raw=True)
    for i, cv in enumerate(convs[1:], 1):
        tp.pack(f"a.conv{i}", cv)
    for i, j in enumerate((0, 2, 4)):
        tp.pack(f"a.fc{i}", vgg.embeddings[j])


def _pack_fusion(tp: TrainPass, m) -> None:
    tp.pack("proj.fc1", m.visual_projector.fc1)
    tp.pack("proj.fc2", m.visual_projector.fc2)
    ca, blk = m.cross_att, m.cross_att.blocks[0]
    tp.pack("ca.pe_v", ca.patch_embed_v.proj)
    tp.pack("ca.pe_a", ca.patch_embed_a.proj)
    rank1 = _RANK1_ATTN and ops.attn1_usable(blk.attn)
    for nme in (("k", "v") if rank1 else ("q", "k", "v", "proj")):   # (the one-key collapse reads attn.q / attn.proj as f32)
        tp.pack("ca." + nme, getattr(blk.attn, nme))
    tp.pack("ca.fc1", blk.mlp.fc1)
    tp.pack("ca.fc2", blk.mlp.fc2)


def _audio_stage(tp: TrainPass, audio: torch.Tensor) -> V:
    """VGGish (vgg.py:17-36) on the tape: [N, 1, 96, 64] f32 -> features [N, latent].  (A ResNet18Audio encoder: _audio18_stage.)"""
    from .cavp_model import VGG, ResNet18Audio
    if isinstance(tp.m.audio_backbone.backbone, ResNet18Audio):
        return _audio18_stage(tp, tp.m.audio_backbone.backbone, audio)
    a = tp.conv_smallcin(audio, "a.conv0", 1, ACT_RELU)
    ci = 1
    for v in VGG.CFG[1:]:
        if v == "M":
            a = tp.maxpool(a, 2, 2, 0)
        else:
            a = tp.conv(a, f"a.conv{ci}", act=ACT_RELU)
            ci += 1
    a = tp.flatten(a)
    a = tp.conv(a, "a.fc0", act=ACT_RELU)
    a = tp.conv(a, "a.fc1", act=ACT_RELU)
    return tp.conv(a, "a.fc2", act=ACT_RELU)


def _fusion_stage(tp: TrainPass, m, fea_v: V, fea_a: V, duplicate: bool):
    """forward_fusion (cavp_model.py:143-154; attn.py:232-244) on the tape.  fea_v NHWC [Bv, h, w, C], fea_a [Ba, C].
    duplicate=True (forward_train): Ba = 2 Bv - the reference duplicates the visual features first (`torch.cat((fea_v,
    fea_v.clone()))`, cavp_model.py:181) and runs projector / patch_embed_v / norm1 / q on both identical halves.  Those four
    GEMMs + LN depend only on fea_v, so they are computed ONCE on Bv rows and their results duplicated where the halves start to
    differ (the audio-conditioned gate); in backward the duplication sums the two halves' gradients - same values, half the
    work.  duplicate=False (the stage entry point): Ba = Bv, row for row.
    Returns (fusion NHWC [Ba, h, w, C], fea_v_proj tokens [Bv, h*w, C], attn)."""
    ca, blk = m.cross_att, m.cross_att.blocks[0]
    Bv, hh, ww, Cc = fea_v.t.shape
    Ba = fea_a.t.shape[0]
    if Ba != (2 * Bv if duplicate else Bv):
        raise CavpError(f"fusion: {Ba} audio feature rows for {Bv} visual maps")
    tokB = tp.reshape(fea_v, (Bv, hh * ww, Cc))
    hidp = tp.conv(tokB, "proj.fc1", act=ACT_GELU) if _FUSE_TOKEN_PATH else tp.gelu(tp.conv(tokB, "proj.fc1"))
    fea_v_projB = tp.conv(hidp, "proj.fc2")
    v0B = tp.conv(fea_v_projB, "ca.pe_v")
    a0 = tp.conv(fea_a, "ca.pe_a")
    vnB = tp.layernorm(v0B, blk.norm1)
    an = tp.layernorm(a0, blk.norm1)
    k = tp.conv(an, "ca.k")
    vv = tp.conv(an, "ca.v")
    if _RANK1_ATTN and ops.attn1_usable(blk.attn):
        # one key per batch item: q-GEMM + gate + proj-GEMM + residual as ONE pass over the tokens (csrc/attn_rank1.hip); the 2B
        # rows of `vn` are never materialised (batch item b reads vn[b % Bv])
        r1, attn = tp.attn_rank1(vnB, k, vv, blk.attn)
        vn = q = o = None
    else:
        qB = tp.conv(vnB, "ca.q")
        # the 2B rows of `vn` / `q` / pack["visual"] are never materialised: the gate reads q[b % B], ca.proj adds the residual row
        # p % (B * T), and the output-only duplicate of fea_v_proj is made by whoever returns it (three 2 x 61 MB copies per step)
        periodic = duplicate and (Bv * hh * ww) % 256 == 0 and _FUSE_TOKEN_PATH
        vn, q = (vnB, qB) if (periodic or not duplicate) else (tp.dup2(vnB), tp.dup2(qB))
        o, attn = tp.attn_gate(q, k, vv, blk.attn.num_heads, blk.attn.scale)
        r1 = tp.conv(o, "ca.proj", residual=vn, residual_periodic=periodic)
    l2 = tp.layernorm(r1, blk.norm2)
    hh2 = tp.conv(l2, "ca.fc1", act=ACT_GELU) if _FUSE_TOKEN_PATH else tp.gelu(tp.conv(l2, "ca.fc1"))
    r2 = tp.conv(hh2, "ca.fc2", residual=r1)
    fus_tok = tp.layernorm(r2, ca.norm)
    fusion = tp.reshape(fus_tok, (Ba, hh, ww, Cc))
    tp.named.update(fusion=fusion, r2=r2, r1=r1, vn=vn, q=q, o=o, fea_v2=fea_v)
    return fusion, fea_v_projB, attn


def _head_stage(tp: TrainPass, m, fusion: V) -> V:
    """Decoder head (encoder_decoder.py:62-75) on the tape: low-resolution logits [N, h, w, Cpad]; channels >= num_classes are
    exact zeros."""
    up = m.segment.upsample
    z0h = tp.conv(fusion, "head0", stats=up.last_conv[1])
    c1 = tp.bn_act(z0h, up.last_conv[1], ACT_RELU)
    z1h = tp.conv(c1, "head1", stats=up.last_conv[4])
    c2 = tp.bn_act(z1h, up.last_conv[4], ACT_RELU)
    lo = tp.conv(c2, "cls")
    tp.named.update(z0h=z0h, c1=c1, z1h=z1h, c2=c2, lo=lo)
    return lo


def run_train_forward(model, image: torch.Tensor, audio: torch.Tensor, tp: TrainPass, shuffle=None, fusion_tap=None):
    """Mirrors CAVP._forward_hip (eval) op by op with batch-statistics BN and a backward tape.  Returns the V's of
    (logits_lowres, fusion NHWC, fea_v_proj NHWC, fea_a, attn).
    fusion_tap: a TrainPass.grad_tap function for the fusion map, recorded between the fusion stage and the head: in the backward
    it runs after head0's data gradient and before the fusion stage's (the contrastive term of the native step enters there)."""
    from .cavp_model import VGG
    m = model
    pvt = m.seg_model == "PVT"
    rn = None if pvt else m.backbone.backbone
    B = image.shape[0]
    if (collectives_on() and tp.dev.type == "cuda" and not torch.cuda.is_current_stream_capturing()
            and any(isinstance(mm, nn.SyncBatchNorm) for mm in m.modules())):
        tp.syncbn_poison = _syncbn_shape_exchange(m, tp.dev, (B, int(image.shape[-2]), int(image.shape[-1])))
    # ---- pack ----
    if not pvt:
        tp.pack("stem0", rn.conv1[0], raw=True)
        tp.pack("stem1", rn.conv1[3])
        tp.pack("stem2", rn.conv1[6])
        for si in range(4):
            for bi, blk in enumerate(getattr(rn, f"layer{si + 1}")):
                key = f"l{si + 1}.{bi}"
                tp.pack(key + ".c1", blk.conv1)
                tp.pack(key + ".c2", blk.conv2)
                tp.pack(key + ".c3", blk.conv3)
                if blk.downsample is not None:
                    tp.pack(key + ".ds", blk.downsample[0])
    aspp = m.segment.aspp
    for i, cv in enumerate(aspp.map_convs):
        tp.pack(f"aspp.map{i}", cv)
    tp.pack("aspp.gp", aspp.global_pooling_conv)
    tp.pack("aspp.pool_red", aspp.pool_red_conv)
    tp.pack("aspp.red", aspp.red_conv)
    tp.pack("reduce", m.segment.reduce[0])
    _pack_head(tp, m)
    _pack_fusion(tp, m)
    n_main = len(tp._pack_jobs)
    _pack_audio(tp, m)
    ev_start = None
    if tp.dev.type == "cuda":   # (the side stream may start once the step's inputs / weights are final: before the main re-pack)
        ev_start = torch.cuda.Event()
        ev_start.record(torch.cuda.current_stream())
    # the audio encoder's re-packs (73 M of the ~115 M weights: the 12288 x 4096 and 4096 x 4096 FC layers) go to the stream that runs
    # the audio encoder - forward and backward - so the main stream only re-packs what it uses itself
    side_packs_on = _SIDE_PACKS and tp.side_stream() is not None and not pvt
    # (also moving the main stream's data-gradient layouts over was measured: no further gain, the weights are then read twice)
    audio_packs = tp.flush_packs(keep_from=n_main if side_packs_on else None)

    dt = tp.dt
    if pvt:
        # ---- PVTv2-B5 backbone (pvt.py:291-306; cavp_amd/pvt_train.py) ----
        from .pvt_train import pvt_train_forward
        feats = pvt_train_forward(tp, m.backbone, image, drop_scales=getattr(m, "_pvt_drop_scales", None))
    else:
        # ---- backbone (resnet.py:186-201) ----
        z = tp.conv_smallcin(image, "stem0", 2, ACT_NONE)
        x = tp.bn_act(z, rn.conv1[1], ACT_RELU)
        x = tp.bn_act(tp.conv(x, "stem1", stats=rn.conv1[4]), rn.conv1[4], ACT_RELU)
        if _FUSE_STEM_POOL:
            x = tp.bn_act(tp.conv(x, "stem2", stats=rn.bn1), rn.bn1, ACT_RELU, pool=(3, 2, 1))
        else:
            x = tp.bn_act(tp.conv(x, "stem2", stats=rn.bn1), rn.bn1, ACT_RELU)
            x = tp.maxpool(x, 3, 2, 1)
        feats = []
        for si, stage in enumerate(rn.block_table):
            for bi, (_, _, _, has_ds) in enumerate(stage):
                blkm = getattr(rn, f"layer{si + 1}")[bi]
                key = f"l{si + 1}.{bi}"
                bs = tp.branch_stream() if has_ds else None
                if bs is not None:   # the block input is final here: the down-sample branch may start
                    ev_x = torch.cuda.Event()
                    ev_x.record(torch.cuda.current_stream())
                o = tp.bn_act(tp.conv(x, key + ".c1", stats=blkm.bn1), blkm.bn1, ACT_RELU)
                o = tp.bn_act(tp.conv(o, key + ".c2", stats=blkm.bn2), blkm.bn2, ACT_RELU)
                if bs is not None:
                    # down-sample conv + BatchNorm (resnet.py:84-90) depend on the block input only: three small launches that run on
                    # a stream of their own beside conv1 -> conv2 (forward only; issued here so that the tape keeps the forward order)
                    bs.wait_event(ev_x)
                    with torch.cuda.stream(bs), ops.workspace_slot(2):
                        tp._slot = 2
                        try:
                            res = tp.bn_act(tp.conv(x, key + ".ds", stats=blkm.downsample[1]), blkm.downsample[1], ACT_NONE)
                        finally:
                            tp._slot = 0
                        ev_r = torch.cuda.Event()
                        ev_r.record(bs)
                    torch.cuda.current_stream().wait_event(ev_r)
                else:
                    res = tp.bn_act(tp.conv(x, key + ".ds", stats=blkm.downsample[1]), blkm.downsample[1], ACT_NONE) if has_ds else x
                x = tp.bn_act(tp.conv(o, key + ".c3", stats=blkm.bn3), blkm.bn3, ACT_RELU, residual=res)
                tp.named[key] = x
            feats.append(x)
    for i, f in enumerate(feats):
        tp.named[f"stage{i + 1}"] = f
    f1, f4 = feats[0], feats[-1]
    # ---- ASPP + skip (encoder_decoder.py:97-105,137-156) ----
    n, h, w, _ = f4.t.shape
    hid = tp.P["aspp.map0"].cout
    zcat = V(tp.empty((n, h, w, 4 * hid)))
    for i in range(4):
        tp.conv(f4, f"aspp.map{i}", out=zcat.slice(i * hid, (i + 1) * hid))
    cat = tp.bn_act(zcat, aspp.map_bn, ACT_LEAKY)
    pool = tp.cast(tp.gap(f4), dt)
    g = tp.bn_act(tp.conv(pool, "aspp.gp"), aspp.global_pooling_bn, ACT_LEAKY)
    g = tp.cast(tp.conv(g, "aspp.pool_red"), torch.float32)
    zred = tp.conv(cat, "aspp.red", nbias=g)
    asp = tp.bn_act(zred, aspp.red_bn, ACT_LEAKY)
    _, lh, lw, _ = f1.t.shape
    co = tp.P["aspp.red"].cout
    fea_v = V(tp.empty((n, lh, lw, co + tp.P["reduce"].cout)))
    tp.bilinear(asp, fea_v.slice(0, co), align_corners=True)
    tp.bn_act(tp.conv(f1, "reduce", stats=True), m.segment.reduce[1], ACT_RELU, out=fea_v.slice(co, co + tp.P["reduce"].cout))
    tp.mark_early_grads_final()   # backward: all parameter gradients of the ops below are final when this is reached
    # ---- audio on 2B (cavp_model.py:181-186; vgg.py:17-23) ----
    if audio.shape[0] != (B if shuffle is not None else 2 * B):
        raise CavpError(f"train mode expects audio of {'B' if shuffle is not None else '2B'} clips (cavp_model.py:181,160-173), "
                        f"got {audio.shape[0]} for {B} images")
    def audio_encoder():
        return _audio_stage(tp, audio)

    # The audio encoder depends on nothing but its input and feeds only the fusion: it runs on a second stream, concurrently
    # with the visual backbone (whose 14 x 14 layers and small BatchNorm kernels leave most of the chip idle), forward and
    # backward.  The kernels are ISSUED after the backbone's but wait only for the weight re-pack (`ev_start`).
    side = tp.side_stream()
    t0 = len(tp.tape)
    if side is None:
        assert not audio_packs
        fea_a = audio_encoder()
    else:
        side.wait_event(ev_start)
        with torch.cuda.stream(side), ops.workspace_slot(1):
            tp._slot = 1
            try:
                T.pack_weights_multi(audio_packs, tp.dt)   # (held back by flush_packs above; the side section's backward runs on this stream too)
                fea_a = audio_encoder()
            finally:
                tp._slot = 0
            ev_audio = torch.cuda.Event()
            ev_audio.record(side)
        torch.cuda.current_stream().wait_event(ev_audio)
        tp.side_range = (t0, len(tp.tape))
    if shuffle is not None:   # forward_audio (cavp_model.py:156-173): features | the same features gathered by shuffle_idx
        fea_a = tp.gather_cat(fea_a, model._bank_and_shuffle(fea_a.t, shuffle[0], shuffle[1]))
    fusion, fea_v_proj, attn = _fusion_stage(tp, m, fea_v, fea_a, duplicate=True)
    if fusion_tap is not None:
        tp.grad_tap(fusion, fusion_tap)
    lo = _head_stage(tp, m, fusion)
    tp.named.update(fea_v=fea_v, f4=f4, f1=f1, fea_a=fea_a, asp=asp, cat=cat, zcat=zcat)
    if tp._nbt:
        bump_counters(model, tp._nbt)   # one launch: the visual path's 61 counters (+ the 20 of a ResNet-18 audio encoder)
        tp._nbt = []
    if tp.syncbn_poison is not None:   # ranks with unequal shapes in this step (_syncbn_shape_exchange): NaN logits -> NaN loss and gradients
        lo.t.add_(tp.syncbn_poison.to(lo.t.dtype))
        tp.syncbn_poison = None
    return lo, fusion, fea_v_proj, fea_a, attn


class _no_gc_during_capture:
    """Python's cyclic collector can run at any allocation - also in the middle of a stream capture - and whatever it finalises then
    (an old hipGraph / graph-exec of an earlier GraphedTrainStep, a stream, a pinned buffer) issues HIP calls that are illegal
    while capturing: the error surfaces in a C++ destructor and aborts the process (seen once in the GPU suite, in a capture that
    followed several captured models).  Collect BEFORE the capture starts, keep the collector off until it has ended."""

    def __enter__(self):
        import gc
        self._was = gc.isenabled()
        gc.collect()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()
        return False


def _private(g: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """`g` (a layout / dtype conversion of the foreign gradient `src`) as memory the tape may accumulate into IN PLACE
    (TrainPass.acc): when the conversion was a no-op, `g` still is the caller's grad_output (autograd forbids mutating it) or a
    static graph buffer (it would carry one replay's data gradient into the next), so it is copied."""
    return g.clone() if g.untyped_storage().data_ptr() == src.untyped_storage().data_ptr() else g


class CAVPTrainFunction(torch.autograd.Function):
    """One autograd node for the whole model: inputs (image, audio, *parameters) -> (out_pred, out_fusion, visual,
    audio_feat, attn_v).  Gradients flow from out_pred and out_fusion."""

    @staticmethod
    def forward(ctx, model, image, audio, *params):
        tp = TrainPass(model, model.compute_dtype)
        with torch.no_grad():
            lo, fusion, fea_v_proj, fea_a, attn = run_train_forward(model, image.contiguous(), audio.contiguous(), tp,
                                                                    shuffle=getattr(model, "_train_shuffle", None))
            model._train_shuffle = None
            B2, C = lo.t.shape[0], model.num_classes
            out_pred = torch.empty((B2, C) + tuple(image.shape[-2:]), dtype=torch.float32, device=image.device)
            ops.bilinear_to_nchw(lo.t[..., :C], out_pred, align_corners=False)
            f32 = model._as_f32
            out_fusion = f32(fusion.t).permute(0, 3, 1, 2)
            vis = f32(fea_v_proj.t).view((-1,) + tuple(fusion.t.shape[1:]))
            visual = torch.cat((vis, vis), dim=0).permute(0, 3, 1, 2)   # cavp_model.py:181: the two halves are identical
            audio_f = f32(fea_a.t)[:, :, None, None]
            attn_v = attn.t.unsqueeze(-1)
        ctx.set_materialize_grads(False)   # an unused output (out_fusion under a CE-only loss) arrives as None, not as 244 MB of zeros
        ctx.tp, ctx.lo, ctx.fusion, ctx.params, ctx.hw = tp, lo, fusion, params, tuple(image.shape[-2:])
        ctx.model_ref = model
        ctx.mark_non_differentiable(visual, audio_f, attn_v)
        return out_pred, out_fusion, visual, audio_f, attn_v

    @staticmethod
    def backward(ctx, d_pred, d_fusion, *_unused):
        tp, lo, fusion = ctx.tp, ctx.lo, ctx.fusion
        with torch.no_grad():
            if d_pred is not None:
                g = T.zeros(lo.t.shape, lo.t.dtype, lo.t.device)
                T.bilinear_bwd_from_nchw(d_pred.contiguous().float(), g[..., :d_pred.shape[1]], n_valid=lo.t.shape[0],
                                         align_corners=False)
                lo.set_g(g)
            if d_fusion is not None:
                gf = d_fusion.permute(0, 2, 3, 1).contiguous().float()   # boundary layout conversion of a foreign tensor
                gf = _private(gf, d_fusion) if fusion.t.dtype == torch.float32 else ops.cast(gf, tp.empty(gf.shape, fusion.t.dtype))
                fusion.set_g(gf)
            tp.backward()
            tp.finish_padded()
        grads = []
        for p in ctx.params:
            g = tp.grads.get(id(p))
            grads.append(None if g is None else g.view(p.shape))
        ctx.model_ref._last_train_pass = tp if getattr(ctx.model_ref, '_keep_train_pass', False) else None
        ctx.model_ref.params_changed()   # the forward updated running_mean / running_var through raw pointers
        ctx.tp = None
        return (None, None, None) + tuple(grads)


class CAVPStageFunction(torch.autograd.Function):
    """The reference's stage entry points (cavp_model.py:138-173) as autograd nodes over a TrainPass tape of that stage only:
    `forward_cls`, `forward_fusion`, `forward_audio` called on a model in training mode (batch-statistics BatchNorm, running
    statistics updated) or with gradients enabled.  inputs = the stage's tensor arguments followed by the trainable parameters;
    `kind` selects the stage, `meta` carries its non-tensor arguments."""

    @staticmethod
    def forward(ctx, model, kind, meta, n_in, *tensors):
        ins, params = tensors[:n_in], tensors[n_in:]
        tp = TrainPass(model, model.compute_dtype)
        dt, dev = tp.dt, tp.dev
        f32 = model._as_f32

        def nhwc(t):   # a caller's NCHW-shaped tensor -> dense NHWC of the compute dtype
            return model._nchw_to_nhwc(t.detach(), dt)

        with torch.no_grad():
            if kind == "cls":
                _pack_head(tp, model)
                tp.flush_packs()
                x = V(nhwc(ins[0]), needs_grad=ins[0].requires_grad)
                lo = _head_stage(tp, model, x)
                C = model.num_classes
                out = torch.empty((lo.t.shape[0], C) + tuple(meta), dtype=torch.float32, device=dev)
                ops.bilinear_to_nchw(lo.t[..., :C], out, align_corners=False)
                ctx.vin, ctx.vout, outs = [x], [lo], (out,)
            elif kind == "fusion":
                _pack_fusion(tp, model)
                tp.flush_packs()
                v = V(nhwc(ins[0]), needs_grad=ins[0].requires_grad)
                a2 = ins[1].detach().reshape(ins[1].shape[0], -1).contiguous()
                a = V(a2 if a2.dtype == dt else ops.cast(a2, torch.empty(a2.shape, dtype=dt, device=dev)),
                      needs_grad=ins[1].requires_grad)
                fusion, proj, attn = _fusion_stage(tp, model, v, a, duplicate=False)
                outs = (f32(fusion.t).permute(0, 3, 1, 2), f32(proj.t).view(fusion.t.shape).permute(0, 3, 1, 2), attn.t.unsqueeze(-1))
                ctx.vin, ctx.vout = [v, a], [fusion, proj]
                ctx.mark_non_differentiable(outs[2])
            elif kind == "audio":
                _pack_audio(tp, model)
                tp.flush_packs()
                fea = _audio_stage(tp, ins[0].detach().contiguous())
                fea = tp.gather_cat(fea, model._bank_and_shuffle(fea.t, meta[0], meta[1]))
                outs = (f32(fea.t),)
                ctx.vin, ctx.vout = [], [fea]
            else:
                raise CavpError(f"unknown stage {kind!r}")
            if tp._nbt:
                bump_counters(model, tp._nbt)
                tp._nbt = []
        model.params_changed()   # batch-statistics BatchNorm wrote running_mean / running_var through raw pointers
        ctx.set_materialize_grads(False)
        ctx.tp, ctx.kind, ctx.params, ctx.n_in, ctx.in_meta = tp, kind, params, n_in, [(t.shape, t.dtype) for t in ins]
        return outs if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *douts):
        tp, kind = ctx.tp, ctx.kind
        if tp is None:
            raise CavpError("a stage's backward can run once (its tape is released afterwards)")
        dt = tp.dt

        def to_nhwc(g0):   # foreign NCHW-shaped gradient -> dense NHWC of the compute dtype, in memory the tape owns
            g = g0.permute(0, 2, 3, 1).contiguous().float()
            return _private(g, g0) if dt == torch.float32 else ops.cast(g, tp.empty(g.shape, dt))

        with torch.no_grad():
            if kind == "cls":
                lo = ctx.vout[0]
                if douts[0] is not None:
                    g = T.zeros(lo.t.shape, lo.t.dtype, lo.t.device)
                    T.bilinear_bwd_from_nchw(douts[0].contiguous().float(), g[..., :douts[0].shape[1]], n_valid=lo.t.shape[0],
                                             align_corners=False)
                    lo.set_g(g)
            elif kind == "fusion":
                fusion, proj = ctx.vout
                if douts[0] is not None:
                    fusion.set_g(to_nhwc(douts[0]))
                if douts[1] is not None:
                    proj.set_g(to_nhwc(douts[1]).view(proj.t.shape))
            else:
                fea = ctx.vout[0]
                if douts[0] is not None:
                    g = douts[0].contiguous().float()
                    fea.set_g(_private(g, douts[0]) if dt == torch.float32 else ops.cast(g, tp.empty(g.shape, dt)))
            tp.backward()
            tp.finish_padded()
            gin = []
            for v, (shape, dtype) in zip(ctx.vin, ctx.in_meta):
                if not v.needs_grad or v.g is None:
                    gin.append(None)
                    continue
                g = v.g if v.g.dtype == torch.float32 else ops.cast(v.g.contiguous(), torch.empty(v.g.shape, dtype=torch.float32,
                                                                                                   device=v.g.device))
                g = g.permute(0, 3, 1, 2) if g.dim() == 4 else g.reshape(shape)
                gin.append(g.to(dtype) if dtype != torch.float32 else g)
            gin += [None] * (ctx.n_in - len(gin))
        grads = []
        for p in ctx.params:
            g = tp.grads.get(id(p))
            grads.append(None if g is None else g.view(p.shape))
        ctx.tp = None
        return (None, None, None, None) + tuple(gin) + tuple(grads)


class GraphedTrainStep:
    """forward_train and its backward as two hipGraphs behind ONE autograd node: the reference's training call sequence
    (`out, fus, pack = model(image, audio)`; a loss on `out` / `fus` built with torch; `loss.backward()`;
    trainer_cavp_vpo_mono.py:166-193) at graph-replay speed instead of ~600 eager launches per direction.

    Graph A = weight re-pack + forward on the tape + the f32 / NCHW output conversions, reading the static `image` / `audio`
    buffers; graph B (same memory pool) = gradient layout conversion + the whole backward, reading static `d_pred` / `d_fusion`
    buffers and leaving every parameter gradient in a flat arena.  torch.autograd runs whatever the caller computes in between.
    The outputs are static buffers too: consume them (and call backward) before the next forward - the usual contract of graphed
    callables.  Captured per (image shape, audio shape) by `CAVP.enable_graphed_autograd`; falls back to the eager node for any
    other shape, for `audio_func=True` and without gradients."""

    def __init__(self, model, image: torch.Tensor, audio: torch.Tensor):
        from .cavp_model import _GRAD_OVERWRITE_MIN
        self.m = model
        self.key = (tuple(image.shape), tuple(audio.shape), model.compute_dtype)
        self.image, self.audio = image.detach().clone().contiguous(), audio.detach().clone().contiguous()
        dev = image.device
        big = {id(mm.weight) for mm in model.modules() if isinstance(mm, (nn.Linear, nn.Conv2d))
               and mm.weight.numel() >= _GRAD_OVERWRITE_MIN} if _GRAD_OVERWRITE_MIN > 0 else set()
        self.arena = GradArena(list(model.parameters()), dev, late_ids=model._late_grad_ids(), no_zero_ids=big)
        B2, C = audio.shape[0] if audio.shape[0] == 2 * image.shape[0] else 2 * image.shape[0], model.num_classes
        self.d_pred = torch.zeros((B2, C) + tuple(image.shape[-2:]), dtype=torch.float32, device=dev)
        self.d_fusion = None      # allocated by the first forward (needs the fusion map's size)
        self._state = None
        # a device DropPath sampler (CAVP.use_device_drop_path): graph A draws the masks itself and reads the sampler's state
        self.dp_sampler = getattr(model.backbone, "_dp_sampler", None) if model.seg_model == "PVT" else None
        # the warm-up passes below run the real kernels: BatchNorm running statistics / counters are put back afterwards
        saved = [(b, b.detach().clone()) for b in model.buffers()]
        with torch.no_grad():
            for _ in range(2):    # warm-up: workspaces, allocator, lazily configured kernels - on a side stream like torch's recipe
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    st = self._forward_body()
                    if self.d_fusion is None:
                        # NHWC memory behind an NCHW-shaped view, like out_fusion itself: the layout pass of the backward is then a no-op
                        n_, c_, h_, w_ = st["out_fusion"].shape
                        self.d_fusion = torch.zeros((n_, h_, w_, c_), dtype=torch.float32, device=dev).permute(0, 3, 1, 2)
                    self._backward_body(st)
                torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.gA, self.gB = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            cap = torch.cuda.Stream()
            cap.wait_stream(torch.cuda.current_stream())
            with _no_gc_during_capture(), torch.cuda.stream(cap):
                self.gA.capture_begin(capture_error_mode="thread_local")
                st = self._forward_body()
                self.gA.capture_end()
                self.gB.capture_begin(pool=self.gA.pool(), capture_error_mode="thread_local")
                self._backward_body(st)
                self.gB.capture_end()
            torch.cuda.current_stream().wait_stream(cap)
            for b, c in saved:
                b.copy_(c)
        self._zeroed = {"d_pred", "d_fusion"}    # static gradient buffers that currently hold zeros
        self.outs = (st["out_pred"], st["out_fusion"], st["visual"], st["audio_f"], st["attn_v"])
        self.touched = st["touched"]
        model.params_changed()

    def _forward_body(self):
        m = self.m
        self.arena.zero()
        tp = TrainPass(m, m.compute_dtype, arena=self.arena)
        lo, fusion, fea_v_proj, fea_a, attn = run_train_forward(m, self.image, self.audio, tp)
        B2, C = lo.t.shape[0], m.num_classes
        out_pred = torch.empty((B2, C) + tuple(self.image.shape[-2:]), dtype=torch.float32, device=self.image.device)
        ops.bilinear_to_nchw(lo.t[..., :C], out_pred, align_corners=False)
        f32 = m._as_f32
        out_fusion = f32(fusion.t).permute(0, 3, 1, 2)
        vis = f32(fea_v_proj.t).view((-1,) + tuple(fusion.t.shape[1:]))
        visual = torch.cat((vis, vis), dim=0).permute(0, 3, 1, 2)
        return dict(tp=tp, lo=lo, fusion=fusion, out_pred=out_pred, out_fusion=out_fusion, visual=visual,
                    audio_f=f32(fea_a.t)[:, :, None, None], attn_v=attn.t.unsqueeze(-1), touched=None)

    def _backward_body(self, st):
        tp, lo, fusion = st["tp"], st["lo"], st["fusion"]
        g = T.zeros(lo.t.shape, lo.t.dtype, lo.t.device)
        T.bilinear_bwd_from_nchw(self.d_pred, g[..., :self.d_pred.shape[1]], n_valid=lo.t.shape[0], align_corners=False)
        lo.set_g(g)
        # (d_fusion is NHWC memory, so this "conversion" is a view of the STATIC buffer: the head's data gradient is accumulated into
        # fusion.g in place, and a replay must not leave it in the buffer the next replay starts from - f32 copies, bf16 casts)
        gf = self.d_fusion.permute(0, 2, 3, 1).contiguous()
        fusion.set_g(_private(gf, self.d_fusion) if fusion.t.dtype == torch.float32 else ops.cast(gf, tp.empty(gf.shape, fusion.t.dtype)))
        tp.backward()
        tp.finish_padded()
        st["touched"] = set(tp.touched)

    def release_adopted(self, params) -> None:
        """p.grad tensors that autograd adopted from the arena (GraphedTrainFunction.backward) and that are still alive get private
        memory before a replay touches the arena again."""
        base = self.arena.flat.untyped_storage().data_ptr()
        for p in params:
            if p.grad is not None and p.grad.untyped_storage().data_ptr() == base:
                p.grad = p.grad.clone()

    def matches(self, image, audio) -> bool:
        return (tuple(image.shape), tuple(audio.shape), self.m.compute_dtype) == self.key and image.device == self.image.device


class GraphedTrainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, step: GraphedTrainStep, image, audio, *params):
        m = step.m
        step.release_adopted(params)      # (graph A starts by clearing the arena)
        step.image.copy_(image)
        step.audio.copy_(audio)
        if m.seg_model == "PVT" and getattr(m, "_pvt_drop_scales", None) is None and step.dp_sampler is None:
            from .pvt_train import refresh_drop_path
            refresh_drop_path(m.backbone, image.shape[0], image.device)   # the graph reads the persistent mask buffer
        step.gA.replay()
        m.params_changed()      # the graph updated the running statistics through raw pointers
        ctx.step, ctx.params = step, params
        ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None in backward, not as a 244 MB zero tensor
        # fresh tensor objects over the static buffers every call (an output object must not carry the previous call's grad_fn)
        out_pred, out_fusion, visual, audio_f, attn_v = (o.detach() for o in step.outs)
        ctx.mark_non_differentiable(visual, audio_f, attn_v)
        return out_pred, out_fusion, visual, audio_f, attn_v

    @staticmethod
    def backward(ctx, d_pred, d_fusion, *_unused):
        step = ctx.step
        # static gradient inputs of graph B; a buffer that is already zero is not cleared again (the trainers' CE-only loss never
        # touches out_fusion: materialised zeros copied into the NHWC buffer were a 320 us strided copy per step)
        for name, g in (("d_pred", d_pred), ("d_fusion", d_fusion)):
            buf = getattr(step, name)
            if g is not None:
                buf.copy_(g)
                step._zeroed.discard(name)
            elif name not in step._zeroed:
                buf.zero_()
                step._zeroed.add(name)
        # The gradients are handed over as FRESH views of the arena: autograd's AccumulateGrad then adopts them as p.grad instead of
        # cloning ~230 tensors (0.8 ms of copy launches per step).  p.grad therefore aliases the arena until the caller drops it
        # (zero_grad(set_to_none=True), the default): a p.grad that still aliases it when the next
        # forward (which clears the arena) or backward starts means the caller accumulates over several passes - release_adopted moves
        # it to private memory first.
        step.release_adopted(ctx.params)
        step.gB.replay()
        grads = tuple(step.arena.views[id(p)].view(p.shape) if id(p) in step.touched else None for p in ctx.params)
        return (None, None, None) + grads
