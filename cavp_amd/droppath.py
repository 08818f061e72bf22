"""DropPath masks of the PVTv2-B5 backbone drawn on the device (csrc/pvt_train.hip): the captured training step of
a PVT model draws its own stochastic-depth masks, so a replay is a pure replay and a skipped step can be rolled back.

    dp = model.use_device_drop_path(seed=0)   # PVT only (CavpError for DeepLabV3Plus); returns this DropPathSampler
    dp.manual_seed(s)                         # seed, offset <- 0, in place: graphs captured earlier see it on their next replay
    dp.offset()                               # synchronises: the number of draws since the last manual_seed()
    rb.add(dp)                                # StepRollback: {seed, offset} through rollback_ranges()
    model.use_device_drop_path(None)          # back to the host draws

Opt-in and additive: without a sampler `pvt_train.draw_drop_path_scales` draws on the host from torch's default CPU generator
exactly as before.  With one, every training forward that needs masks is ONE launch of `cavp_drop_path_draw` on the current
stream: all rows of the [n, B] factor table (one row per residual branch with p > 0, in forward order) from the device state
{seed, offset}, then offset += 1.  While a hipGraph is being captured the launch writes the persistent `backbone._dp_buf` and
becomes part of the graph - every replay draws fresh masks, and neither `capture_train_step`'s replay() nor the graphed autograd
node touches the host generator.  An eager pass writes a fresh private table, so a later forward cannot change the masks of a
pending backward.  backbone.eval(), a model whose probabilities are all 0 and a `_pvt_drop_scales` override launch nothing and
leave the offset alone.

The rule (the specification; tests/_droppath_ref.py restates it in numpy):
    r = Philox4x32-10(counter = (sample b, branch row k, offset_lo, offset_hi), key = (seed_lo, seed_hi))
    u = (r[0] >> 8) * 2^-24                                   # 24 bits, [0, 1)
    out[k, b] = inv_keep[k] if keep[k] + u >= 1 else 0        # the sum in f32: timm 0.4.9's floor(keep + rand) / keep
with keep = float32(1 - p) and inv_keep = float32(1) / keep computed on the host as the host path computes them.  The
distribution is the reference's (a branch survives with probability keep, to 2^-24), the stream is not: no seed reproduces
torch's CPU draws, as with FrameAugment.

Data-parallel runs: every rank must draw its own masks, so each rank passes its own seed - the reference seeds its generators
with `seed_it(hyp_param.seed + hyp_param.local_rank)` (main_*.py), which is `model.use_device_drop_path(seed=seed + local_rank)` here."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import torch

from . import _lib
from .ops import _ptr, _stream

MAX_ELEMENTS = 1 << 20        # n * B of one launch (cavp_drop_path_draw)


class DropPathSampler:
    """See the module docstring.  The constructor touches no device: the state is allocated by the first draw (or by offset() /
    rollback_ranges()), on `device` or else on the device of that draw."""

    def __init__(self, seed: int = 0, device=None):
        self._device = device
        self._seed = 0
        self._state = None
        self._tables: Dict[Tuple[float, ...], Tuple[torch.Tensor, torch.Tensor]] = {}
        self.manual_seed(seed)

    # ---- device state (the layout of FrameAugment's: int64 {seed, offset} at the head of the block) ------------------------------
    def _ensure(self, device=None):
        if self._state is None:
            dev = self._device if self._device is not None else device
            dev = torch.device(dev) if dev is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("DropPathSampler lives on a HIP device (there is no CPU fallback)")
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            if torch.cuda.is_current_stream_capturing():
                raise _lib.CavpError("DropPathSampler: the first draw cannot be inside a capture (run a warm-up pass first)")
            self.device = dev
            self._state = torch.zeros(2, dtype=torch.int64, device=dev)
            self.manual_seed(self._seed)
        return self._state

    def manual_seed(self, seed: int) -> None:
        """Reset the seed and the draw counter (offset 0).  A host-to-device write: not legal during a capture; graphs captured
        earlier see the new values on their next replay."""
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._seed = s - (1 << 64) if s >= (1 << 63) else s
        if self._state is not None:
            self._state[:2].copy_(torch.tensor([self._seed, 0], dtype=torch.int64))

    def rollback_ranges(self):
        """[(name, tensor, byte_offset, nbytes)]: {seed, offset}, the only state a draw mutates.  For StepRollback.add()."""
        return [("state", self._ensure(), 0, 16)]

    def offset(self) -> int:
        """Synchronises: the number of draws (eager passes and replays) since the last manual_seed()."""
        return int(self._ensure()[1].item())

    # ---- the draw ------------------------------------------------------------------------------------------------------------
    def _tables_for(self, probs: Tuple[float, ...], dev):
        tab = self._tables.get(probs)
        if tab is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.CavpError("DropPathSampler: the keep table of this model is not on the device yet and cannot be "
                                     "uploaded inside a capture (run a warm-up pass first)")
            # the host path's values: keep = float32(1 - p), and ones / keep is what its floor_().div_(keeps) yields for a kept sample
            keep = torch.tensor([1.0 - p for p in probs], dtype=torch.float32)
            tab = self._tables[probs] = (keep.to(dev), (torch.ones_like(keep) / keep).to(dev))
        return tab

    def draw(self, probs, B: int, out: torch.Tensor) -> torch.Tensor:
        """One launch on the current stream: out (f32 [n, B], dense, on the sampler's device) <- the factors of the n branches with
        the drop probabilities `probs` (each in (0, 1)) at the current offset; offset += 1."""
        probs = tuple(float(p) for p in probs)
        n, B = len(probs), int(B)
        if n < 1 or B < 1 or n * B > MAX_ELEMENTS or any(not 0.0 < p < 1.0 for p in probs):
            raise _lib.CavpError(f"DropPathSampler: n = {n} branches x B = {B} outside [1, 2^20] or a probability outside (0, 1)")
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (n, B) \
                or not out.is_contiguous():
            raise _lib.CavpError(f"DropPathSampler: out must be a dense float32 [{n}, {B}] device tensor")
        state = self._ensure(out.device)
        if out.device != self.device:
            raise _lib.CavpError(f"DropPathSampler lives on {self.device}, out on {out.device}")
        keep, inv = self._tables_for(probs, self.device)
        _lib.check(_lib.load().cavp_drop_path_draw(_ptr(state), _ptr(keep), _ptr(inv), n, B, _ptr(out), C.c_void_p(_stream())),
                   "cavp_drop_path_draw")
        return out
