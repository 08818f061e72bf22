"""StepRollback: a skipped step also undoes what its forward wrote (csrc/rollback.hip).

`StepGuard` keeps the weights, the optimiser state and the step counter where they were when a gradient or a loss is not finite.
By then the forward has already written every BatchNorm's running statistics and counter, pushed clips into the pair builder's
sound bank and advanced the call counters of the pair builder, the frame augmentation and the anchor sampler.  A StepRollback
holds a device-resident table of those byte ranges and a shadow arena of the same size:

    rb = StepRollback(device)
    rb.add_model(model)        # running_mean / running_var / num_batches_tracked of every tracking BatchNorm
    rb.add(pairs)              # PairBuilder: bank, ring heads, {seed, offset}      (bank=False leaves the bank out)
    rb.add(augment)            # FrameAugment: {seed, offset}
    rb.add(crit)               # ContrastLoss device sampler: {seed, offset}
    rb.add(dp)                 # DropPathSampler (PVT, model.use_device_drop_path): {seed, offset}
    rb.add_tensor(t)           # anything else
    rb.freeze()                # the table and the shadow arena (one allocation); no add*() after it
    replay = model.capture_train_step(..., optimizer=opt, prologue=prologue, rollback=rb)

or, eagerly, `rb.save(); model.train_step(...); opt.step(losses=...); rb.restore_if_skipped(guard)`.  save() is one launch that
copies every range into its shadow, restore_if_skipped() one launch that loads the guard's `skip` word on the device and copies
the shadows back when it is set - every workgroup leaves after that one load when it is not.  Nothing but stats() synchronises and
everything can be captured.

Not rolled back, on purpose: the diagnostic counters (`bad_inputs` of the pair builder and the augmentation, the sampler's
`dropped_classes` and bad-label count, LabelStage / WaveStage state) - a skipped step must not hide that its input was bad -
and output or scratch buffers, which are not state.

The registered tensors must keep their storage: `load_state_dict`, `manual_seed` and `load_bank` write in place and are fine, a
`model.to(...)` or a re-allocated buffer after freeze() is not."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from .ops import _ptr, _stream

ROLLBACK_SCRUB = 1          # CAVP_ROLLBACK_SCRUB
BLOCK_BYTES = 1024          # the unit of cavp_rollback_blocks
SPAN_BLOCKS = 16            # blocks one workgroup serves per pass: a span of 16 KiB


class RollbackRange(C.Structure):
    """struct cavp_rollback_range (include/cavp_hip.h)."""
    _fields_ = [("live", C.c_void_p), ("shadow", C.c_void_p), ("nbytes", C.c_int64), ("blk0", C.c_int32), ("flags", C.c_int32)]


class RollbackState(C.Structure):
    """struct cavp_rollback_state (include/cavp_hip.h)."""
    _fields_ = [("saves", C.c_int64), ("restores", C.c_int64)]


def bn_state_tensors(model: nn.Module) -> List[Tuple[str, torch.Tensor]]:
    """(name, buffer) of running_mean, running_var and num_batches_tracked of every BatchNorm / SyncBatchNorm module that tracks
    running statistics and has the buffers: the modules whose buffers the training forward hands to the finalize kernels.
    Independent of `.training`: a frozen layer's buffers are never written, so saving and restoring them changes nothing."""
    out = []
    for name, m in model.named_modules():
        if not isinstance(m, nn.modules.batchnorm._BatchNorm) or not m.track_running_stats or m.running_mean is None:
            continue
        prefix = name + "." if name else ""
        out.append((prefix + "running_mean", m.running_mean))
        out.append((prefix + "running_var", m.running_var))
        if m.num_batches_tracked is not None:
            out.append((prefix + "num_batches_tracked", m.num_batches_tracked))
    return out


def build_table(entries, shadow_base: int):
    """The table of `entries` = [(live address, nbytes, flags)] in the given order with the shadows laid out from `shadow_base`
    (16-byte aligned): every shadow starts at the first address at or above the previous one's end that has its live range's
    offset from a 16-byte boundary, so each range takes the 16-byte path.  Scrub ranges have no shadow.  Returns
    (ctypes array of RollbackRange, total_blocks, shadow bytes).  Pure host arithmetic."""
    lib = _lib.load()
    tab = (RollbackRange * max(len(entries), 1))()
    blk, cur = 0, 0
    for i, (live, nbytes, flags) in enumerate(entries):
        shadow = None
        if not flags & ROLLBACK_SCRUB:
            off = (cur + 15) // 16 * 16 + (live & 15)
            shadow, cur = shadow_base + off, off + nbytes
        tab[i] = RollbackRange(live, shadow, nbytes, blk, flags)
        blk += int(lib.cavp_rollback_blocks(C.c_int64(live), C.c_int64(nbytes)))
        if blk >= 1 << 31:
            raise _lib.CavpError("StepRollback: more than 2^31 blocks of 1 KiB registered")
    return tab, blk, (cur + 15) // 16 * 16


class StepRollback:
    """See the module docstring.  `device`: the HIP device every registered tensor lives on.  The constructor and the add*()
    calls touch no device; freeze() allocates the table, the state block and the shadow arena."""

    def __init__(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.CavpError("StepRollback lives on a HIP device (there is no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.device = dev
        self._entries: List[Tuple[int, int, int]] = []   # (live address, nbytes, flags)
        self._groups: List[str] = []                     # per entry: the group it was registered under
        self._keep: List[torch.Tensor] = []
        self._frozen = False
        self._table = self._state = self._arena = None
        self.total_blocks = 0

    # ---- registration ------------------------------------------------------------------------------------------------------
    def _add_raw(self, live: int, nbytes: int, flags: int, group: str) -> None:
        """The checks that need no tensor: multiples of 4, no range twice, no overlap."""
        if self._frozen:
            raise _lib.CavpError("StepRollback: frozen; register every range before freeze()")
        if nbytes <= 0 or nbytes % 4 or live % 4:
            raise _lib.CavpError(f"StepRollback: a range must be a positive multiple of 4 bytes at a 4-byte aligned address "
                                 f"(got {nbytes} bytes at offset {live % 16} from a 16-byte boundary)")
        for (a, n, _), g in zip(self._entries, self._groups):
            if a == live and n == nbytes:
                raise _lib.CavpError(f"StepRollback: this range is already registered (under '{g}')")
            if live < a + n and a < live + nbytes:
                raise _lib.CavpError(f"StepRollback: the range overlaps one registered under '{g}'")
        self._entries.append((live, nbytes, flags))
        self._groups.append(group)

    def _check_tensor(self, t, what: str) -> None:
        if not torch.is_tensor(t):
            raise _lib.CavpError(f"StepRollback.{what}: a tensor is required")
        if not t.is_contiguous():
            raise _lib.CavpError(f"StepRollback.{what}: the tensor must be contiguous")
        if not t.is_cuda:
            raise _lib.CavpError(f"StepRollback.{what}: a CPU tensor; the rollback needs HIP device tensors (no CPU fallback)")
        if t.device != self.device:
            raise _lib.CavpError(f"StepRollback.{what}: the rollback lives on {self.device}, the tensor on {t.device}")

    def add_tensor(self, t: torch.Tensor, byte_offset: int = 0, nbytes: Optional[int] = None, *, group: str = "tensors") -> "StepRollback":
        """Register `nbytes` bytes of a contiguous device tensor from `byte_offset` on (default: all of it)."""
        self._check_tensor(t, "add_tensor")
        total = t.numel() * t.element_size()
        nbytes = total - int(byte_offset) if nbytes is None else int(nbytes)
        if int(byte_offset) < 0 or nbytes < 0 or int(byte_offset) + nbytes > total:
            raise _lib.CavpError("StepRollback.add_tensor: the byte range leaves the tensor")
        self._add_raw(t.data_ptr() + int(byte_offset), nbytes, 0, group)
        self._keep.append(t)
        return self

    def add_scrub(self, t: torch.Tensor, *, group: str = "scrub") -> "StepRollback":
        """Register a workspace that a restore fills with zeros (nothing of it is saved): for a buffer the step reads before it
        writes, where a non-finite value of a poisoned iteration would otherwise reach the next one."""
        self._check_tensor(t, "add_scrub")
        self._add_raw(t.data_ptr(), t.numel() * t.element_size(), ROLLBACK_SCRUB, group)
        self._keep.append(t)
        return self

    def add_model(self, model: nn.Module) -> "StepRollback":
        """Every tracking BatchNorm's running_mean, running_var and num_batches_tracked (bn_state_tensors)."""
        for _, t in bn_state_tensors(model):
            self.add_tensor(t, group="model")
        return self

    def add(self, stage, **kw) -> "StepRollback":
        """A stage that names its own state through `rollback_ranges()`: PairBuilder (`bank=False` leaves the sound bank out),
        FrameAugment, ContrastLoss with the device sampler, the feeders, PVT's DropPathSampler."""
        fn = getattr(stage, "rollback_ranges", None)
        if fn is None:
            raise _lib.CavpError(f"StepRollback.add: {type(stage).__name__} has no rollback_ranges(); use add_tensor")
        for name, t, off, n in fn(**kw):
            self.add_tensor(t, off, n, group=f"{type(stage).__name__}.{name}")
        return self

    def registered_bytes(self) -> Dict[str, int]:
        """Bytes per group (the model, each stage field, loose tensors, scrub ranges), in registration order."""
        out: Dict[str, int] = {}
        for (_, n, _), g in zip(self._entries, self._groups):
            out[g] = out.get(g, 0) + n
        return out

    def ranges(self) -> List[torch.Tensor]:
        """uint8 views of the live ranges that are saved, in table order: for tests and checkpoints of the registered state."""
        self._need_frozen("ranges()")
        return [v for v, (_, _, f) in zip(self._views, self._entries) if not f & ROLLBACK_SCRUB]

    # ---- the device side ------------------------------------------------------------------------------------------------------
    def freeze(self) -> "StepRollback":
        """Build the device table, the state block and the shadow arena (one allocation).  An empty rollback is legal: its
        save() and restore() are no-ops."""
        if self._frozen:
            raise _lib.CavpError("StepRollback.freeze: already frozen")
        lib = _lib.load()
        if lib.cavp_rollback_range_bytes() != C.sizeof(RollbackRange) or lib.cavp_rollback_state_bytes() != C.sizeof(RollbackState):
            raise _lib.CavpError("StepRollback: the library's cavp_rollback_range / cavp_rollback_state and their mirrors differ in size")
        _, _, shadow_bytes = build_table(self._entries, 0)
        self._arena = torch.empty(max(shadow_bytes, 16), dtype=torch.uint8, device=self.device)
        tab, self.total_blocks, _ = build_table(self._entries, self._arena.data_ptr())
        self._table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
        self._state = torch.zeros(C.sizeof(RollbackState), dtype=torch.uint8, device=self.device)
        # uint8 views of the live ranges (_keep holds the tensor of each entry, which also keeps it alive)
        self._views = []
        for (live, n, _), owner in zip(self._entries, self._keep):
            off = live - owner.data_ptr()
            self._views.append(owner.view(-1).view(torch.uint8)[off:off + n])
        self._frozen = True
        return self

    def _need_frozen(self, what: str) -> None:
        if not self._frozen:
            raise _lib.CavpError(f"StepRollback.{what}: call freeze() first")

    def save(self) -> None:
        """One launch on the current stream: every range into its shadow."""
        self._need_frozen("save()")
        _lib.check(_lib.load().cavp_rollback_save(_ptr(self._table), len(self._entries), self.total_blocks, _ptr(self._state),
                                                  C.c_void_p(_stream())), "cavp_rollback_save")

    def _restore(self, word) -> None:
        _lib.check(_lib.load().cavp_rollback_restore(_ptr(self._table), len(self._entries), self.total_blocks, word,
                                                     _ptr(self._state), C.c_void_p(_stream())), "cavp_rollback_restore")

    def restore(self) -> None:
        """One launch: every shadow back into its range and zeros into the scrub ranges, unconditionally."""
        self._need_frozen("restore()")
        self._restore(None)

    def restore_if_skipped(self, guard) -> None:
        """One launch behind a guarded `opt.step(losses=...)` on the same stream: the restore happens when the guard's `skip`
        word is set, which the guard writes on every guarded step.  Nothing is read back."""
        from .optim import GuardState, StepGuard
        if not isinstance(guard, StepGuard):
            raise _lib.CavpError("StepRollback.restore_if_skipped: a cavp_amd.optim.StepGuard is required")
        if guard._buf is None:
            raise _lib.CavpError("StepRollback.restore_if_skipped: the guard is not attached (FusedSGDAdam.use_step_guard)")
        if guard._buf.device != self.device:
            raise _lib.CavpError(f"StepRollback.restore_if_skipped: the rollback lives on {self.device}, the guard on {guard._buf.device}")
        self._need_frozen("restore_if_skipped()")
        self._restore(C.c_void_p(guard._buf.data_ptr() + GuardState.skip.offset))

    def reset_stats(self) -> None:
        """Zero the two counters: one fill on the current stream, no synchronisation."""
        self._need_frozen("reset_stats()")
        self._state.zero_()

    def stats(self) -> Dict[str, int]:
        """Synchronises once: {saves, restores} - the save launches, and the restores that happened (word set, or forced)."""
        self._need_frozen("stats()")
        s = RollbackState.from_buffer_copy(self._state.cpu().numpy().tobytes())
        return {"saves": int(s.saves), "restores": int(s.restores)}
