"""Optimiser side of the training harness ("caller/harness rows"), MI355X-native.

The reference drives the model with two torch optimisers (main_vpo_mono.py:45-65,118-125):
  * SGD(momentum, weight_decay) over `set_group_lr(model)`: backbone {decay, no-decay} at lr, visual_projector and
    cross_att (all parameters, default weight decay) at lr, each of the four `segment.business_layer` modules
    {decay, no-decay} at 10 x lr - where `group_weight` (engine/utils.py:642-688) puts conv / linear weights in the decay
    group and their biases plus every norm-layer parameter in the no-decay (weight_decay = 0) group;
  * Adam over `audio_backbone` at the constant base lr;
and a warm-up + polynomial learning-rate schedule (engine/lr_policy.py:30-43, trainer lr_step :73-85).

Because `cavp_amd.cavp_model.CAVP` keeps the reference's module tree, those torch optimisers work on it unchanged.  This
module is the fused alternative for `CAVP.train_step`: every parameter is updated by ONE kernel launch
(`cavp_optimizer_step`) straight from the flat gradient arena, with a device-resident job table built once.

`FusedSGDAdam.use_device_schedule(...)` moves the step counter and the schedule to the GPU as well (struct cavp_opt_state):
`step()` is then two launches that take nothing from the host, and `CAVP.capture_train_step(optimizer=...)` records them at
the end of the training graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib
from .ops import _ptr, _stream

_NORMS = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.GroupNorm, nn.LayerNorm)   # SyncBatchNorm is a BatchNorm subclass
_CONVS = (nn.Conv1d, nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d)


def group_weight(groups: List[dict], module: nn.Module, lr: float) -> List[dict]:
    """engine/utils.py:642-688: [weights of conv / linear] at `lr` with the optimiser's weight decay, [their biases +
    all norm-layer parameters] at `lr` with weight_decay = 0.  Raises if a parameter of `module` is in neither set (the
    reference asserts the same)."""
    decay, no_decay = [], []
    for m in module.modules():
        if isinstance(m, (nn.Linear,) + _CONVS):
            decay.append(m.weight)
            if m.bias is not None:
                no_decay.append(m.bias)
        elif isinstance(m, _NORMS):
            if m.weight is not None:
                no_decay.append(m.weight)
            if m.bias is not None:
                no_decay.append(m.bias)
    if len(list(module.parameters())) != len(decay) + len(no_decay):
        raise _lib.CavpError("group_weight: a parameter outside Linear / Conv / norm layers (engine/utils.py:685)")
    groups.append(dict(params=decay, lr=lr))
    groups.append(dict(params=no_decay, weight_decay=0.0, lr=lr))
    return groups


def set_group_lr(model, lr: float, use_baseline: bool = False) -> List[dict]:
    """main_vpo_mono.py:45-65.  Group order (the trainer's lr_step indexes it): 0-1 backbone, 2 projector, 3 cross
    attention, 4.. decoder modules at 10 x lr."""
    groups: List[dict] = []
    group_weight(groups, model.backbone, lr)
    if not use_baseline:
        groups.append({"params": list(model.visual_projector.parameters()), "lr": lr})
        groups.append({"params": list(model.cross_att.parameters()), "lr": lr})
    for module in model.segment.business_layer:
        group_weight(groups, module, lr * 10.0)
    return groups


def warmup_poly_lr(start_lr: float, lr_power: float, total_iters: int, warmup_steps: int = 0,
                   end_lr: float = 1e-8) -> Callable[[int], float]:
    """engine/lr_policy.py:30-43 (WarmUpPolyLR.get_lr)."""
    total = float(total_iters)

    def get_lr(cur_iter: int) -> float:
        if cur_iter < warmup_steps:
            return start_lr * (cur_iter / warmup_steps)
        lr = start_lr * ((1.0 - float(cur_iter) / total) ** lr_power)
        return float(min(max(lr, end_lr), start_lr))
    return get_lr


class OptJob(C.Structure):
    """struct cavp_opt_job (include/cavp_hip.h)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("lr_mult", C.c_float), ("weight_decay", C.c_float), ("blk0", C.c_int32), ("kind", C.c_int32),
                ("vec", C.c_int32), ("pad_", C.c_int32)]


class OptState(C.Structure):
    """struct cavp_opt_state (include/cavp_hip.h)."""
    _fields_ = [("t", C.c_int64), ("total_iters", C.c_int64), ("warmup_steps", C.c_int64), ("start_lr", C.c_double),
                ("lr_power", C.c_double), ("end_lr", C.c_double), ("base_lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("lr_sgd", C.c_float), ("lr_adam", C.c_float), ("bc1", C.c_float),
                ("bc2_sqrt", C.c_float), ("first_step", C.c_int32)]


class GuardState(C.Structure):
    """struct cavp_guard_state (include/cavp_hip.h)."""
    _fields_ = [("max_norm", C.c_float), ("skip_nonfinite", C.c_int32), ("history", C.c_int32), ("skip", C.c_int32),
                ("grad_norm", C.c_float), ("norm_sgd", C.c_float), ("norm_adam", C.c_float), ("clip_coef", C.c_float),
                ("nonfinite", C.c_int64), ("skipped_total", C.c_int64), ("head", C.c_int64)]


class StepRecord(C.Structure):
    """struct cavp_step_record (include/cavp_hip.h)."""
    _fields_ = [("t", C.c_int64), ("nonfinite", C.c_int64), ("l_ce", C.c_float), ("l_ctr", C.c_float), ("lr_sgd", C.c_float),
                ("grad_norm", C.c_float), ("clip_coef", C.c_float), ("flags", C.c_int32)]


STEP_SKIPPED, STEP_CLIPPED, STEP_NO_LOSS, STEP_NO_LOSS1, STEP_SKIPPED_LOSS = 1, 2, 4, 8, 16   # CAVP_STEP_* (cavp_step_record.flags)
GUARD_SKIP_GRADIENTS, GUARD_SKIP_LOSSES = 1, 2   # CAVP_GUARD_SKIP_* (cavp_guard_state.skip_nonfinite)


class StepGuard:
    """Gradient norm, `clip_grad_norm_` clipping, a skip of the whole update on a non-finite gradient and a ring of per-step
    records, all on the device (struct cavp_guard_state): the safety and the eyes of a captured iteration, which has no host in
    its loop.  Attach it with `FusedSGDAdam.use_step_guard(guard)`; `opt.step(losses=...)` is then four launches (block partials
    of the gradients' squares, their fixed-order combine in double, the guarded schedule, the guarded update).

    max_norm: None = measure only; otherwise the 2-norm bound of torch.nn.utils.clip_grad_norm_ over every gradient the update
        reads, coefficient min(1, max_norm / (norm + 1e-6)).  Unlike torch the gradient arena is NOT rescaled: the update takes
        coefficient x g and `p.grad` keeps the raw gradient.
    skip_nonfinite: when a gradient element is NaN / inf or the norm is not finite (finite gradients whose squares overflow f32
        count), the step does not happen.  With skip_nonfinite=False a NaN gradient goes into the update, and with clipping a
        NaN norm gives coefficient 1.
    skip_nonfinite_loss: a switch of its own - the step is also skipped when a loss handed to `step(losses=...)` is not finite.
        (The CE head answers a batch whose labels are all ignored with a NaN loss and ZERO gradients: momentum and weight decay
        would move the weights on a batch that said nothing.)  Such a skip carries `skipped_on_loss` in its record.  A loss is
        the caller's value, not the reduced arena's: data parallel it is rank-local, so `capture_train_step` refuses a guard with
        this switch on while collectives are on, and an eager caller must hand every rank the same (reduced) losses.
    A skipped step leaves untouched: parameters, the momentum buffer, Adam's two moment buffers, the step counter t and
        therefore the next learning rate.  NOT rolled back unless a `StepRollback` is attached (cavp_amd/rollback.py,
        `capture_train_step(rollback=)`): BatchNorm running statistics, the sound bank and the call counters of the pair builder
        and the anchor sampler - the forward has already run.  On its own a skip thus protects the weights; it does not protect
        BatchNorm buffers from a non-finite *input*.
    history: capacity of the record ring; `read()` reports how many records were overwritten before it saw them.
    Data parallel: the guard runs behind the late all-reduce on the reduced arena, so the gradient rule and the coefficient are
    the same on every rank (the loss rule is not, see above); this is not exercised beyond one process."""

    FIELDS = ("t", "l_ce", "l_ctr", "lr", "grad_norm", "clip_coef", "nonfinite", "skipped", "clipped", "skipped_on_loss")

    def __init__(self, max_norm: Optional[float] = None, skip_nonfinite: bool = True, history: int = 1024,
                 skip_nonfinite_loss: bool = True):
        self.max_norm = self._check_max_norm(max_norm)
        if isinstance(history, bool) or not isinstance(history, int) or not 1 <= history <= (1 << 24):
            raise _lib.CavpError("StepGuard: history must be an int in [1, 2^24]")
        self.skip_nonfinite, self.skip_nonfinite_loss, self.history = bool(skip_nonfinite), bool(skip_nonfinite_loss), history
        self._buf = None      # device: cavp_guard_state + the ring, once attached
        self._partials = None
        self._read_head = 0

    @staticmethod
    def _check_max_norm(x) -> Optional[float]:
        if x is None:
            return None
        import math
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x <= 0:
            raise _lib.CavpError("StepGuard: max_norm must be None or a finite number > 0")
        return float(x)

    def _attach(self, total_blocks: int, device) -> None:
        lib = _lib.load()
        if lib.cavp_guard_state_bytes() != C.sizeof(GuardState) or lib.cavp_step_record_bytes() != C.sizeof(StepRecord):
            raise _lib.CavpError("StepGuard: the library's cavp_guard_state / cavp_step_record and their mirrors differ in size")
        host = bytearray(C.sizeof(GuardState) + self.history * C.sizeof(StepRecord))
        bits = (GUARD_SKIP_GRADIENTS if self.skip_nonfinite else 0) | (GUARD_SKIP_LOSSES if self.skip_nonfinite_loss else 0)
        host[:C.sizeof(GuardState)] = bytes(GuardState(max_norm=self.max_norm or 0.0, skip_nonfinite=bits, history=self.history,
                                                       clip_coef=1.0))
        self._buf = torch.frombuffer(host, dtype=torch.uint8).to(device)
        self._partials = torch.zeros(total_blocks * 8, dtype=torch.uint8, device=device)   # cavp_guard_partial per block
        self._read_head = 0

    def _view(self, field: str, dtype) -> torch.Tensor:
        f = getattr(GuardState, field)
        return self._buf[f.offset:f.offset + f.size].view(dtype)

    def _need_attached(self, what: str):
        if self._buf is None:
            raise _lib.CavpError(f"StepGuard.{what}: attach the guard first (FusedSGDAdam.use_step_guard)")

    def last(self) -> Dict[str, torch.Tensor]:
        """1-element device views of the most recent step's fields; does not synchronise."""
        self._need_attached("last()")
        f32, i64, i32 = torch.float32, torch.int64, torch.int32
        return {"grad_norm": self._view("grad_norm", f32), "norm_sgd": self._view("norm_sgd", f32),
                "norm_adam": self._view("norm_adam", f32), "clip_coef": self._view("clip_coef", f32),
                "nonfinite": self._view("nonfinite", i64), "skip": self._view("skip", i32),
                "skipped_total": self._view("skipped_total", i64), "head": self._view("head", i64)}

    def set_max_norm(self, max_norm: Optional[float]) -> None:
        """Host-to-device write, legal where FusedSGDAdam.set_iteration is: not during a capture, nor while a graph that uses the
        guard is replaying.  Graphs captured earlier clip with the new bound on their next replay."""
        self.max_norm = self._check_max_norm(max_norm)
        if self._buf is not None:
            self._view("max_norm", torch.float32).copy_(torch.tensor([self.max_norm or 0.0], dtype=torch.float32))

    def _set_skipped_total(self, n: int) -> None:
        self._view("skipped_total", torch.int64).copy_(torch.tensor([int(n)], dtype=torch.int64))

    def read(self) -> Dict[str, object]:
        """Synchronises once.  The records written since the previous read(), oldest first, as numpy arrays under FIELDS (plus
        `flags`), and `dropped`: how many more were written in between and overwritten before this call."""
        self._need_attached("read()")
        import numpy as np
        raw = self._buf.cpu().numpy().tobytes()
        state = GuardState.from_buffer_copy(raw[:C.sizeof(GuardState)])
        ring = np.frombuffer(raw, dtype=np.dtype(StepRecord), count=self.history, offset=C.sizeof(GuardState))
        head = int(state.head)
        first = max(self._read_head, head - self.history)
        rec = ring[np.arange(first, head, dtype=np.int64) % self.history]
        out = {"t": rec["t"].copy(), "l_ce": rec["l_ce"].copy(), "l_ctr": rec["l_ctr"].copy(), "lr": rec["lr_sgd"].copy(),
               "grad_norm": rec["grad_norm"].copy(), "clip_coef": rec["clip_coef"].copy(), "nonfinite": rec["nonfinite"].copy(),
               "skipped": (rec["flags"] & STEP_SKIPPED) != 0, "clipped": (rec["flags"] & STEP_CLIPPED) != 0,
               "skipped_on_loss": (rec["flags"] & STEP_SKIPPED_LOSS) != 0,
               "flags": rec["flags"].copy(), "dropped": first - self._read_head}
        self._read_head = head
        return out


class FusedSGDAdam:
    """SGD(momentum, weight_decay) on `set_group_lr(model)` + Adam(lr = base lr) on `model.audio_backbone`, fused.

    `arena` is the model's flat gradient arena (`CAVP.train_step` creates it; gradients are its views).  `step(lr)`
    takes the current learning rate of the poly schedule: the visual groups use lr x {1, 10} (trainer lr_step), the
    audio Adam keeps the constant base lr (trainer_cavp_vpo_mono.py:84 only logs it).

    After `use_device_schedule(...)` the step count, the schedule and Adam's bias corrections live on the device: `step()`
    takes no argument, reads nothing back and can be recorded in a hipGraph (CAVP.capture_train_step(optimizer=...))."""

    def __init__(self, model, arena, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4,
                 use_baseline: bool = False, betas=(0.9, 0.999), eps: float = 1e-8):
        self.base_lr, self.momentum, self.betas, self.eps = float(lr), float(momentum), betas, float(eps)
        self._steps = 0
        self._arena = arena          # capture_train_step checks that the optimiser reads the capturing model's arena
        self._sched = None           # device cavp_opt_state (uint8 tensor) once use_device_schedule() was called
        self._guard = None           # StepGuard once use_step_guard() was called
        import weakref
        self._model = weakref.ref(model) if hasattr(model, "params_changed") else (lambda: None)
        dev = arena.flat.device
        specs = []   # (param, kind, lr_mult, wd)
        for g in set_group_lr(model, 1.0, use_baseline):
            for p in g["params"]:
                specs.append((p, 0, float(g["lr"]), float(g.get("weight_decay", weight_decay))))
        for p in model.audio_backbone.parameters():
            specs.append((p, 1, 1.0, 0.0))                       # torch.optim.Adam default weight_decay = 0
        seen = set()
        for p, *_ in specs:
            if id(p) in seen:
                raise _lib.CavpError("FusedSGDAdam: a parameter appears in two groups")
            seen.add(id(p))
        # torch.optim skips parameters whose .grad is None: cross_att.pos_embed_v / pos_embed_a and audio_backbone.cls_head never
        # receive a gradient on this path (cavp_model.py / attn.py:235-238), so they get neither weight decay nor momentum
        never = {id(p) for p in getattr(model, "params_without_grad", lambda: [])()}
        specs = [s for s in specs if s[0].requires_grad and id(s[0]) in arena.views and id(s[0]) not in never]
        # state: one flat buffer for momentum / first moments, one for Adam's second moments
        offs, tot = [], 0
        for p, *_ in specs:
            offs.append(tot)
            tot += (p.numel() + 3) // 4 * 4
        self.state_m = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.state_v = torch.zeros(tot, dtype=torch.float32, device=dev)
        lib = _lib.load()
        jobs = (OptJob * len(specs))()
        blk = 0
        self._keep = []
        for i, ((p, kind, lr_mult, wd), off) in enumerate(zip(specs, offs)):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise _lib.CavpError("FusedSGDAdam: contiguous f32 parameters on the arena's device required")
            g = arena.views[id(p)]
            m = self.state_m[off:off + p.numel()]
            v = self.state_v[off:off + p.numel()]
            vec = int(all(t.data_ptr() % 16 == 0 for t in (p, g, m)))
            jobs[i] = OptJob(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr_mult, wd, blk, kind, vec, 0)
            blk += lib.cavp_optimizer_blocks(p.numel())
            self._keep.append(p)
        self.njobs, self.total_blocks = len(specs), blk
        raw = bytes(jobs)
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)   # device-resident job table
        self.params = [s[0] for s in specs]

    # ---- device-resident schedule ----------------------------------------------------------------------------------------
    def use_device_schedule(self, start_lr: float, lr_power: float, total_iters: int, warmup_steps: int = 0,
                            end_lr: float = 1e-8) -> "FusedSGDAdam":
        """Keep the step counter t, the warm-up + poly schedule (`warmup_poly_lr` with these arguments) and Adam's bias
        corrections on the device.  Step t runs with the configured rate for t == 0 and with get_lr(t - 1) afterwards (the
        reference sets the rate after the step, trainer_cavp_vpo_mono.py:193-203); get_lr(i) for i >= total_iters, where the
        host function has no value, is `end_lr`.  The counter starts at the number of steps taken so far."""
        if int(total_iters) < 1 or int(warmup_steps) < 0:
            raise _lib.CavpError("use_device_schedule: total_iters >= 1 and warmup_steps >= 0 required")
        lib = _lib.load()
        if lib.cavp_optimizer_state_bytes() != C.sizeof(OptState):
            raise _lib.CavpError("use_device_schedule: struct cavp_opt_state of the library and OptState differ in size")
        b1, b2 = self.betas
        host = OptState(t=self._steps, total_iters=int(total_iters), warmup_steps=int(warmup_steps), start_lr=float(start_lr),
                        lr_power=float(lr_power), end_lr=float(end_lr), base_lr=self.base_lr, beta1=b1, beta2=b2,
                        lr_sgd=float(start_lr), lr_adam=self.base_lr, bc1=1.0, bc2_sqrt=1.0, first_step=0)
        self._sched = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.state_m.device)
        self._t_view = self._sched[OptState.t.offset:OptState.t.offset + 8].view(torch.int64)
        self._lr_view = self._sched[OptState.lr_sgd.offset:OptState.lr_sgd.offset + 4].view(torch.float32)
        return self

    def use_step_guard(self, guard: "StepGuard") -> "FusedSGDAdam":
        """Attach a StepGuard: `step(losses=...)` then measures the gradient norm, clips, skips a non-finite step and writes one
        record per step, all on the device (four launches, nothing read back).  Needs the device schedule.  Attach it before
        capturing: a graph recorded earlier keeps the unguarded pair of launches."""
        if not isinstance(guard, StepGuard):
            raise _lib.CavpError("use_step_guard: a cavp_amd.optim.StepGuard is required")
        self._need_sched("use_step_guard()")
        if self._guard is not None:
            raise _lib.CavpError("use_step_guard: this optimiser already has a guard")
        if guard._buf is not None:
            raise _lib.CavpError("use_step_guard: the guard is attached to another optimiser")
        guard._attach(self.total_blocks, self.state_m.device)
        self._guard = guard
        return self

    @property
    def steps(self) -> int:
        """Completed steps.  With the device schedule this is `iteration()` and synchronises."""
        return self.iteration() if self._sched is not None else self._steps

    @steps.setter
    def steps(self, n: int) -> None:
        if self._sched is not None:
            self.set_iteration(n)
        else:
            self._steps = int(n)

    def _need_sched(self, what: str):
        if self._sched is None:
            raise _lib.CavpError(f"FusedSGDAdam.{what} needs the device schedule (use_device_schedule)")

    def last_lr(self) -> torch.Tensor:
        """1-element f32 device view of the SGD rate of the most recent step (the rate of the start before the first one).
        A trainer logs lr_bkb = lr_attn = lr, lr_seg = 10 lr and lr_audio = base_lr from it when it chooses to synchronise."""
        self._need_sched("last_lr()")
        return self._lr_view

    def iteration(self) -> int:
        """t, the number of completed steps, read from the device: synchronises, so never call it during a capture."""
        self._need_sched("iteration()")
        return int(self._t_view.item())

    def set_iteration(self, t: int) -> None:
        """Host-to-device write of t.  Like ContrastLoss.manual_seed it is not legal during a capture, nor while a graph that
        uses the state is replaying; graphs captured earlier see the new value on their next replay."""
        self._need_sched("set_iteration()")
        if int(t) < 0:
            raise _lib.CavpError("set_iteration: t >= 0 required")
        self._t_view.copy_(torch.tensor([int(t)], dtype=torch.int64))

    @staticmethod
    def _loss_ptrs(losses, dev):
        if losses is None:
            return None, None
        if torch.is_tensor(losses) or not isinstance(losses, (tuple, list)) or len(losses) > 2:
            raise _lib.CavpError("FusedSGDAdam.step(losses=...): a tuple of up to two 1-element f32 device tensors")
        for t in losses:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != 1 or t.device != dev:
                raise _lib.CavpError("FusedSGDAdam.step(losses=...): a tuple of up to two 1-element f32 device tensors")
        return (_ptr(losses[0]) if len(losses) > 0 else None), (_ptr(losses[1]) if len(losses) > 1 else None)

    def step(self, lr: Optional[float] = None, losses=None) -> None:
        """One update from the arena's gradients.  `step(lr)` takes the rate of the host schedule; with the device schedule
        `step()` issues the schedule launch and the update launch on the current stream and reads nothing back.  With a
        StepGuard attached it issues the guard's four launches instead; `losses` (up to two 1-element f32 device tensors,
        l_ce and l_ctr) go into the step's record."""
        if losses is not None and self._guard is None:
            raise _lib.CavpError("FusedSGDAdam.step(losses=...): no StepGuard attached (use_step_guard)")
        if self._sched is not None and lr is not None:
            raise _lib.CavpError("FusedSGDAdam.step(lr): the schedule lives on the device (use_device_schedule); call step()")
        if self._sched is None and lr is None:
            raise _lib.CavpError("FusedSGDAdam.step(): no learning rate; pass step(lr) or call use_device_schedule() first")
        l0, l1 = self._loss_ptrs(losses, self.state_m.device)
        if self._model() is not None:
            self._model().params_changed()   # weights change through raw pointers: no tensor version is bumped
        if self._guard is not None:
            lib, st, gd = _lib.load(), C.c_void_p(_stream()), self._guard
            tab, nj, nb = _ptr(self.table), self.njobs, self.total_blocks
            _lib.check(lib.cavp_grad_guard_partials(tab, nj, nb, _ptr(gd._partials), st), "cavp_grad_guard_partials")
            _lib.check(lib.cavp_grad_guard_finish(tab, nj, nb, _ptr(gd._partials), _ptr(gd._buf), st), "cavp_grad_guard_finish")
            _lib.check(lib.cavp_optimizer_schedule_guarded(_ptr(self._sched), _ptr(gd._buf), l0, l1, st),
                       "cavp_optimizer_schedule_guarded")
            _lib.check(lib.cavp_optimizer_step_guarded(tab, nj, nb, C.c_float(self.momentum), C.c_float(self.eps),
                                                       _ptr(self._sched), _ptr(gd._buf), st), "cavp_optimizer_step_guarded")
            return
        if self._sched is not None:
            lib, st = _lib.load(), C.c_void_p(_stream())
            _lib.check(lib.cavp_optimizer_schedule(_ptr(self._sched), st), "cavp_optimizer_schedule")
            _lib.check(lib.cavp_optimizer_step_dev(_ptr(self.table), self.njobs, self.total_blocks, C.c_float(self.momentum),
                                                   C.c_float(self.eps), _ptr(self._sched), st), "cavp_optimizer_step_dev")
            return
        self._steps += 1
        b1, b2 = self.betas
        st = _lib.load().cavp_optimizer_step(_ptr(self.table), self.njobs, self.total_blocks, C.c_float(lr),
                                             C.c_float(self.base_lr), C.c_float(self.momentum), C.c_float(b1),
                                             C.c_float(b2), C.c_float(self.eps), C.c_int64(self._steps),
                                             C.c_void_p(_stream()))
        _lib.check(st, "cavp_optimizer_step")

    def state_dict(self) -> Dict[str, object]:
        sd = {"steps": self.steps, "m": self.state_m.clone(), "v": self.state_v.clone()}
        if self._sched is not None:
            sd["t"] = sd["steps"]
        if self._guard is not None:
            sd["guard"] = {"skipped_total": int(self._guard.last()["skipped_total"].item()), "max_norm": self._guard.max_norm}
        return sd

    def load_state_dict(self, sd) -> None:
        """`steps` / `t`, `m`, `v`; and the guard's `skipped_total` and `max_norm` when both sides have a guard.  Intended: a
        `guard` entry loaded into an optimiser without a guard is ignored (a guarded run's checkpoint continues unguarded),
        and a dict without the entry leaves an attached guard's counter and bound as they are."""
        self.steps = int(sd["t"]) if "t" in sd else int(sd["steps"])
        self.state_m.copy_(sd["m"])
        self.state_v.copy_(sd["v"])
        if self._guard is not None and "guard" in sd:
            self._guard.set_max_norm(sd["guard"]["max_norm"])
            self._guard._set_skipped_total(sd["guard"]["skipped_total"])
