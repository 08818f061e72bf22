"""Gradient accumulation in the captured step: N micro-batches per optimiser update (csrc/grad_accum.hip + the gated twins of the
optimiser's launches in csrc/optimizer.hip).

    opt = FusedSGDAdam(model, model.grad_arena(dev), lr).use_device_schedule(...)   # a StepGuard is optional, as without this
    acc = GradAccumulator(opt, micro_steps=8)
    replay = model.capture_train_step(image, audio, label, optimizer=opt, accumulate=acc, ...)
    for _ in range(windows * 8):
        ...copy / feed the next micro-batch...
        replay()          # 7 of 8 replays only accumulate; the 8th also guards, schedules and updates

Accumulating the gradients of N micro-batches and stepping once gives the arithmetic of N data-parallel ranks with local
BatchNorm, up to summation order: each micro-batch normalises with its own statistics, the update sees sum_k g_k / N (the
micro-steps run with loss_scale / N), and the schedule advances once per window.

The rules (restated in numpy in tests/_accumulate_ref.py), with g the arena after micro-step k of a window of N:
    k == 0           acc <- g          a copy: nothing of an earlier window survives, NaNs of a skipped window included
    0 < k < N - 1    acc <- acc + g
    k == N - 1       g   <- acc + g    the window's sum goes back into the arena: the guard's norm, the clip, the update and
                                       `p.grad` read it where they read gradients without accumulation
    N == 1           the arena is left alone and the accumulator is never touched
one IEEE f32 add per element and micro-step, in micro-step order - torch's `.grad` accumulation over N calls of
`(loss / N).backward()`.  After a micro-step `p.grad` therefore holds that micro-step's gradient when it did not close its window
and the window's sum when it did.  Parameters outside the optimiser's job table are not accumulated.
Up to two loss words are summed the same way (sum <- k == 0 ? l : sum + l) and the window's means sum / N, correctly rounded,
are what a StepGuard's record carries as l_ce / l_ctr; the closing micro-step's record is the only record of its window.
A micro-step that does not close its window writes nothing but the accumulator and this module's state block: no record, no
`skipped_total`, the guard's `skip` / `grad_norm` / `clip_coef` keep the last window's values, and t, the rate, the bias
corrections, the parameters and both state buffers are untouched.  A closing micro-step runs exactly the optimiser's guarded or
unguarded launches on the summed arena: same scalars, same bits.
Schedule: t counts WINDOWS, so `total_iters` and `warmup_steps` of `use_device_schedule` are in windows.  A window the guard skips
does not advance t, as without accumulation, and the next window starts clean.

Out of scope: data-parallel runs (an all-reduce per micro-step is the wrong design; that needs DDP's `no_sync`), a StepRollback
across a window (its shadow holds one replay) and the autograd-node routes (`enable_graphed_autograd`)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .ops import _ptr, _stream
from .optim import FusedSGDAdam

MAX_MICRO_STEPS = 1 << 16


class AccumState(C.Structure):
    """struct cavp_accum_state (include/cavp_hip.h)."""
    _fields_ = [("n", C.c_int32), ("k", C.c_int32), ("gate", C.c_int32), ("pad_", C.c_int32), ("windows", C.c_int64),
                ("micro_total", C.c_int64), ("loss_sum0", C.c_float), ("loss_sum1", C.c_float), ("loss_mean0", C.c_float),
                ("loss_mean1", C.c_float)]


class GradAccumulator:
    """N = `micro_steps` micro-batches per update of `optimizer` (a FusedSGDAdam with the device schedule; its StepGuard, if any,
    is attached before or after this, but before the capture).  Owns a flat f32 accumulator with the arena's layout (`flat`,
    `nbytes`) and the device state block (struct cavp_accum_state).  An optimiser has at most one accumulator."""

    def __init__(self, optimizer: FusedSGDAdam, micro_steps: int):
        if not isinstance(optimizer, FusedSGDAdam):
            raise _lib.CavpError("GradAccumulator: a cavp_amd.optim.FusedSGDAdam is required")
        if isinstance(micro_steps, bool) or not isinstance(micro_steps, int) or not 1 <= micro_steps <= MAX_MICRO_STEPS:
            raise _lib.CavpError(f"GradAccumulator: micro_steps must be an int in [1, {MAX_MICRO_STEPS}]")
        if getattr(optimizer, "_sched", None) is None:
            raise _lib.CavpError("GradAccumulator: the optimiser needs the device schedule (FusedSGDAdam.use_device_schedule): "
                                 "the window's gate lives on the device and step(lr) cannot be gated")
        if getattr(optimizer, "_accum", None) is not None:
            raise _lib.CavpError("GradAccumulator: this optimiser already has an accumulator")
        lib = _lib.load()
        if lib.cavp_accum_state_bytes() != C.sizeof(AccumState):
            raise _lib.CavpError("GradAccumulator: struct cavp_accum_state of the library and AccumState differ in size")
        arena = optimizer._arena.flat
        if arena.dtype != torch.float32 or not arena.is_contiguous() or arena.data_ptr() % 16:
            raise _lib.CavpError("GradAccumulator: a contiguous, 16-byte aligned f32 gradient arena is required")
        lo, hi = arena.data_ptr(), arena.data_ptr() + 4 * arena.numel()
        for p in optimizer.params:   # the kernel addresses the accumulator by the gradient's offset in the arena
            g = optimizer._arena.views[id(p)]
            if not lo <= g.data_ptr() <= g.data_ptr() + 4 * g.numel() <= hi:
                raise _lib.CavpError("GradAccumulator: a gradient of the optimiser's job table lies outside its arena")
        self.optimizer, self.micro_steps = optimizer, micro_steps
        self.flat = torch.zeros_like(arena)
        self.nbytes = 4 * self.flat.numel()
        host = AccumState(n=micro_steps, k=0)
        self._state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(arena.device)
        self._k_view = self._field("k", torch.int32)
        optimizer._accum = self

    def _field(self, name: str, dtype) -> torch.Tensor:
        f = getattr(AccumState, name)
        return self._state[f.offset:f.offset + f.size].view(dtype)

    # ---- the launches ------------------------------------------------------------------------------------------------------
    def _calls(self, losses=None) -> List[Tuple[str, tuple]]:
        """(entry point, arguments without the stream) of one micro-step, in issue order: the accumulate launch, the state
        advance, then the gated twins of what `optimizer.step()` issues.  At most two launches more than the step without
        accumulation."""
        opt = self.optimizer
        guard = opt._guard
        if losses is not None and guard is None:
            raise _lib.CavpError("GradAccumulator.step(losses=...): no StepGuard attached (FusedSGDAdam.use_step_guard)")
        l0, l1 = opt._loss_ptrs(losses, self.flat.device)
        st = _ptr(self._state)
        gate = C.c_void_p(self._state.data_ptr() + AccumState.gate.offset)
        tab, nj, nb = _ptr(opt.table), opt.njobs, opt.total_blocks
        mom, eps, sched = C.c_float(opt.momentum), C.c_float(opt.eps), _ptr(opt._sched)
        calls = [("cavp_grad_accumulate", (tab, nj, nb, _ptr(opt._arena.flat), _ptr(self.flat), st)),
                 ("cavp_accum_advance", (st, l0, l1))]
        if guard is None:
            calls += [("cavp_optimizer_schedule_gated", (sched, gate)),
                      ("cavp_optimizer_step_dev_gated", (tab, nj, nb, mom, eps, sched, gate))]
            return calls
        # the window's record carries the window's means: the guarded schedule reads them where it reads the step's losses
        base = self._state.data_ptr()
        m0 = C.c_void_p(base + AccumState.loss_mean0.offset) if l0 is not None else None
        m1 = C.c_void_p(base + AccumState.loss_mean1.offset) if l1 is not None else None
        part, gbuf = _ptr(guard._partials), _ptr(guard._buf)
        calls += [("cavp_grad_guard_partials_gated", (tab, nj, nb, part, gate)),
                  ("cavp_grad_guard_finish_gated", (tab, nj, nb, part, gbuf, gate)),
                  ("cavp_optimizer_schedule_guarded_gated", (sched, gbuf, m0, m1, gate)),
                  ("cavp_optimizer_step_guarded_gated", (tab, nj, nb, mom, eps, sched, gbuf, gate))]
        return calls

    def launch_names(self) -> List[str]:
        """The entry points one micro-step issues, in order (no launch happens)."""
        return [name for name, _ in self._calls()]

    def step(self, losses=None) -> None:
        """One micro-step on the current stream, with no host read: the eager form, and what `capture_train_step(accumulate=)`
        records.  The arena holds the micro-step's gradients; for an eager window of N call
        `model.train_step(..., loss_scale=s / N)` and then this.  `losses`: up to two 1-element f32 device tensors (l_ce,
        l_ctr), only with a StepGuard; their window means go into the window's record."""
        calls = self._calls(losses)
        model = self.optimizer._model()
        if model is not None:
            model.params_changed()   # a closing micro-step changes the weights through raw pointers
        lib, stream = _lib.load(), C.c_void_p(_stream())
        for name, args in calls:
            _lib.check(getattr(lib, name)(*args, stream), name)

    # ---- host side ---------------------------------------------------------------------------------------------------------
    def read(self) -> Dict[str, object]:
        """One synchronising read: k (index of the next micro-step in its window), windows, micro_total and window_losses (the
        last closed window's two means; zeros before the first, and for a loss word that was never given)."""
        s = AccumState.from_buffer_copy(self._state.cpu().numpy().tobytes())
        return {"k": int(s.k), "windows": int(s.windows), "micro_total": int(s.micro_total),
                "window_losses": (float(s.loss_mean0), float(s.loss_mean1))}

    def reset(self) -> None:
        """k = 0: the next micro-step opens a window (and, being a copy, drops what the accumulator holds).  A host-to-device
        write, legal where FusedSGDAdam.set_iteration is: not during a capture, nor while a graph that uses the state replays."""
        self._set_k(0)

    def _set_k(self, k: int) -> None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.CavpError("GradAccumulator: k cannot be written during a capture")
        self._k_view.copy_(torch.tensor([int(k)], dtype=torch.int32))

    def state_dict(self) -> Dict[str, object]:
        """The accumulator and k (synchronises), so that a run can resume inside a window; the optimiser's own state_dict
        carries t, m and v."""
        sd = self.read()
        return {"micro_steps": self.micro_steps, "k": sd["k"], "windows": sd["windows"], "micro_total": sd["micro_total"],
                "acc": self.flat.clone(), "loss_sums": torch.stack([self._field("loss_sum0", torch.float32)[0],
                                                                    self._field("loss_sum1", torch.float32)[0]]).cpu()}

    def load_state_dict(self, sd) -> None:
        if int(sd["micro_steps"]) != self.micro_steps:
            raise _lib.CavpError(f"GradAccumulator.load_state_dict: saved with micro_steps = {int(sd['micro_steps'])}, this one "
                                 f"has {self.micro_steps}: a window cannot be resumed at another length")
        if not 0 <= int(sd["k"]) < self.micro_steps or tuple(sd["acc"].shape) != tuple(self.flat.shape):
            raise _lib.CavpError("GradAccumulator.load_state_dict: k or the accumulator's size does not fit")
        self._set_k(int(sd["k"]))
        self.flat.copy_(sd["acc"])
        self._field("windows", torch.int64).copy_(torch.tensor([int(sd["windows"])], dtype=torch.int64))
        self._field("micro_total", torch.int64).copy_(torch.tensor([int(sd["micro_total"])], dtype=torch.int64))
        sums = sd["loss_sums"].to(torch.float32)
        self._field("loss_sum0", torch.float32).copy_(sums[0:1])
        self._field("loss_sum1", torch.float32).copy_(sums[1:2])


def check_capture(accumulate, optimizer, rollback, collectives: bool) -> Optional[int]:
    """The refusals of `capture_train_step(accumulate=)`; returns N (None without an accumulator)."""
    if accumulate is None:
        return None
    if not isinstance(accumulate, GradAccumulator):
        raise _lib.CavpError("capture_train_step: accumulate must be a cavp_amd.accumulate.GradAccumulator")
    if optimizer is None:
        raise _lib.CavpError("capture_train_step: accumulate= needs optimizer=: the window's last replay is the update")
    if accumulate.optimizer is not optimizer:
        raise _lib.CavpError("capture_train_step: the accumulator belongs to another optimiser")
    if rollback is not None:
        raise _lib.CavpError("capture_train_step: rollback= cannot be combined with accumulate=: a window spans several replays "
                             "and the rollback's shadow holds one")
    if collectives:
        raise _lib.CavpError("capture_train_step: accumulate= with collectives on would all-reduce every micro-step; "
                             "data-parallel accumulation (no_sync) is not built")
    return accumulate.micro_steps
