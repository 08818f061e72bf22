"""The step guard on the GPU (struct cavp_guard_state; cavp_grad_guard_partials / _finish, cavp_optimizer_schedule_guarded /
_step_guarded; StepGuard + FusedSGDAdam.use_step_guard): norms against float64, non-finite detection and the skip, the idle
guard against the unguarded optimiser, clipping against torch, skip-and-recover, the record ring, the captured step and the
all-ignored batch end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import _step_guard_ref as R
from tests.test_gpu_optim_sched import (CAP, CFG2, CFG3, SHORT, _op_model, _sgd_adam_split, _state, _with_optimizer, _worst, host_lr,
                                        within_one_ulp)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------------------------------- hand-built job table
# The sizes at which the kernels can go wrong: below / at / above one float4, one element short of a block, a block, a block + 1
# (the last element alone in its workgroup), several blocks + a tail; plus two views that start one float past a 16-byte
# boundary (vec = 0: scalar path), one of them longer than a block.  Kinds alternate, so both are present with and without tails.
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 2]
UNALIGNED = [4101, 7]
IDX_4097 = LENGTHS.index(4097)
IDX_UNALIGNED = len(LENGTHS)
CONSTS = (1e-2, 0.9, 100, 0, 1e-8)


class Table:
    """A job table over raw tensors (no model): gradient views in one flat arena, parameters and both state buffers beside it."""

    def __init__(self, seed=0, scale=0.1):
        from cavp_amd import _lib
        from cavp_amd.optim import OptJob
        lib = _lib.load()
        gen = torch.Generator(device=DEV).manual_seed(seed)
        lens = LENGTHS + UNALIGNED
        offs, tot = [], 0
        for i, n in enumerate(lens):
            tot = (tot + 3) // 4 * 4 + (1 if i >= IDX_UNALIGNED else 0)
            offs.append(tot)
            tot += n
        tot = (tot + 3) // 4 * 4
        self.arena = torch.randn(tot, generator=gen, device=DEV) * scale
        assert self.arena.data_ptr() % 16 == 0
        self.g = [self.arena[o:o + n] for o, n in zip(offs, lens)]
        self.p = [torch.randn(n + 4, generator=gen, device=DEV)[:n] for n in lens]
        self.m = [torch.randn(n + 4, generator=gen, device=DEV)[:n] * 0.1 for n in lens]
        self.v = [torch.rand(n + 4, generator=gen, device=DEV)[:n] * 0.01 for n in lens]
        self.kinds = [i % 2 for i in range(len(lens))]
        jobs = (OptJob * len(lens))()
        blk = 0
        for i, n in enumerate(lens):
            vec = int(all(t.data_ptr() % 16 == 0 for t in (self.p[i], self.g[i], self.m[i])))
            assert vec == (0 if i >= IDX_UNALIGNED else 1)
            jobs[i] = OptJob(self.p[i].data_ptr(), self.g[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), n,
                             1.0 + i, 1e-3, blk, self.kinds[i], vec, 0)
            blk += lib.cavp_optimizer_blocks(n)
        self.njobs, self.total_blocks = len(lens), blk
        self.table = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(DEV)

    def snapshot(self):
        return [[t.clone() for t in ts] for ts in (self.p, self.m, self.v)]

    def reference(self, **kw):
        return R.guard_step([g.cpu().numpy() for g in self.g], self.kinds, **kw)


def _guard(tab, **kw):
    from cavp_amd.optim import StepGuard
    g = StepGuard(**kw)
    g._attach(tab.total_blocks, torch.device(DEV))
    return g


def _sched(t=0):
    from cavp_amd.optim import OptState
    start, power, total, warm, end = CONSTS
    host = OptState(t=t, total_iters=total, warmup_steps=warm, start_lr=start, lr_power=power, end_lr=end, base_lr=1e-3, beta1=0.9,
                    beta2=0.999, lr_sgd=start, lr_adam=1e-3, bc1=1.0, bc2_sqrt=1.0, first_step=0)
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)


def _measure(tab, guard):
    """the two norm launches"""
    from cavp_amd import _lib
    from cavp_amd.ops import _ptr, _stream
    lib, st = _lib.load(), C.c_void_p(_stream())
    _lib.check(lib.cavp_grad_guard_partials(_ptr(tab.table), tab.njobs, tab.total_blocks, _ptr(guard._partials), st), "partials")
    _lib.check(lib.cavp_grad_guard_finish(_ptr(tab.table), tab.njobs, tab.total_blocks, _ptr(guard._partials), _ptr(guard._buf), st),
               "finish")


def _update(tab, guard, sched, loss=None):
    """the guarded schedule and the guarded update"""
    from cavp_amd import _lib
    from cavp_amd.ops import _ptr, _stream
    lib, st = _lib.load(), C.c_void_p(_stream())
    _lib.check(lib.cavp_optimizer_schedule_guarded(_ptr(sched), _ptr(guard._buf), _ptr(loss), None, st), "schedule_guarded")
    _lib.check(lib.cavp_optimizer_step_guarded(_ptr(tab.table), tab.njobs, tab.total_blocks, C.c_float(0.9), C.c_float(1e-8),
                                               _ptr(sched), _ptr(guard._buf), st), "step_guarded")


def _fields(guard):
    from cavp_amd.optim import GuardState
    return GuardState.from_buffer_copy(guard._buf.cpu().numpy().tobytes()[:C.sizeof(GuardState)])


def _sched_fields(sched):
    from cavp_amd.optim import OptState
    return OptState.from_buffer_copy(sched.cpu().numpy().tobytes())


def test_norms_against_float64():
    """grad_norm, norm_sgd, norm_adam within 2e-6 relative of float64.  Squares are non-negative, so an f32 summation tree of L
    levels is off by at most L 2^-24 relative; the bar allows 32 levels (1.9e-6 on the sum, half that on the norm) and the kernel
    uses 12, with everything above the 4096-element block in double.  Two runs on the same arena give equal bits."""
    tab = Table(seed=1)
    guard = _guard(tab, max_norm=None)
    _measure(tab, guard)
    got, part1, buf1 = _fields(guard), guard._partials.clone(), guard._buf.clone()
    ref = tab.reference()
    for name in ("grad_norm", "norm_sgd", "norm_adam"):
        rel = abs(getattr(got, name) - ref[name]) / ref[name]
        print(f"{name}: {getattr(got, name):.9e} (float64 {ref[name]:.9e}), relative {rel:.2e}")
        assert rel <= 2e-6, (name, rel)
    assert got.nonfinite == 0 and got.skip == 0 and got.clip_coef == 1.0
    assert got.max_norm == 0.0 and got.skip_nonfinite == 3 and got.history == 1024 and got.head == 0 and got.skipped_total == 0
    guard._partials.fill_(0xff)
    _measure(tab, guard)
    torch.cuda.synchronize()
    assert torch.equal(guard._partials, part1) and torch.equal(guard._buf, buf1)


# (job, element): element 0 of the table; the last element of the 4097-long tensor, alone in its block; inside the unaligned
# scalar path (second block of the long unaligned view); the last element of the last job
PLACES = {"first": (0, 0), "alone_in_block": (IDX_4097, 4096), "unaligned": (IDX_UNALIGNED, 4098),
          "last": (len(LENGTHS) + len(UNALIGNED) - 1, UNALIGNED[-1] - 1)}


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("place", list(PLACES))
def test_nonfinite_element_skips_the_step(place, value):
    tab = Table(seed=2)
    guard, sched = _guard(tab, max_norm=1.0), _sched(t=3)
    job, el = PLACES[place]
    tab.g[job][el] = value
    before, sched_before = tab.snapshot(), sched.clone()
    _measure(tab, guard)
    _update(tab, guard, sched)
    got = _fields(guard)
    assert got.nonfinite == 1 and got.skip == 1, (got.nonfinite, got.skip)
    assert got.skipped_total == 1 and got.head == 1
    for was, now in zip(before, (tab.p, tab.m, tab.v)):
        assert all(torch.equal(a, b) for a, b in zip(was, now))
    assert torch.equal(sched, sched_before)                     # t, the rates, the bias corrections, first_step


def test_overflowing_squares_skip_and_clean_gradients_update():
    """Finite gradients of 3e19: no element is non-finite, the f32 squares are +inf, the norm is not finite -> skip.  The same table
    with its clean gradients is updated (the control: the skip above is not an update that never runs)."""
    tab = Table(seed=3)
    guard, sched = _guard(tab), _sched(t=0)
    clean = tab.g[2].clone()
    tab.g[2].fill_(3e19)
    before = tab.snapshot()
    _measure(tab, guard)
    _update(tab, guard, sched)
    got = _fields(guard)
    assert got.nonfinite == 0 and math.isinf(got.grad_norm) and got.skip == 1
    for was, now in zip(before, (tab.p, tab.m, tab.v)):
        assert all(torch.equal(a, b) for a, b in zip(was, now))
    assert _sched_fields(sched).t == 0
    tab.g[2].copy_(clean)
    _measure(tab, guard)
    _update(tab, guard, sched)
    got = _fields(guard)
    assert got.skip == 0 and got.skipped_total == 1 and got.head == 2 and _sched_fields(sched).t == 1
    assert all(not torch.equal(a, b) for a, b in zip(before[0], tab.p))
    assert all(torch.isfinite(p).all() for p in tab.p)


@pytest.mark.parametrize("switch", [True, False], ids=["loss_rule_on", "loss_rule_off"])
def test_nonfinite_loss_has_its_own_switch(switch):
    """Clean gradients, a NaN loss.  skip_nonfinite_loss on: skipped, flagged as a skip on the loss, nothing moves - also with the
    gradient rule off.  Off: the loss is recorded, the update runs and t advances."""
    from cavp_amd.optim import STEP_SKIPPED, STEP_SKIPPED_LOSS, StepRecord
    tab = Table(seed=4)
    guard, sched = _guard(tab, skip_nonfinite=False, skip_nonfinite_loss=switch, history=2), _sched(t=0)
    before = tab.snapshot()
    loss = torch.full((1,), float("nan"), device=DEV)
    _measure(tab, guard)
    _update(tab, guard, sched, loss=loss)
    got = _fields(guard)
    raw = guard._buf.cpu().numpy().tobytes()
    rec = StepRecord.from_buffer_copy(raw[C.sizeof(type(got)):C.sizeof(type(got)) + C.sizeof(StepRecord)])
    assert got.nonfinite == 0 and math.isnan(rec.l_ce) and rec.t == 0
    moved = [not torch.equal(a, b) for a, b in zip(before[0], tab.p)]
    if switch:
        assert got.skip == 1 and got.skipped_total == 1 and rec.flags & STEP_SKIPPED and rec.flags & STEP_SKIPPED_LOSS
        assert not any(moved) and _sched_fields(sched).t == 0
    else:
        assert got.skip == 0 and got.skipped_total == 0 and not rec.flags & (STEP_SKIPPED | STEP_SKIPPED_LOSS)
        assert all(moved) and _sched_fields(sched).t == 1


# ------------------------------------------------------------------------------------------------------------ on the op model
def _pair(guard_kw, consts=CONSTS):
    """(model, arena, guarded optimiser, guard) and (model, arena, unguarded device-schedule optimiser) on identical parameters"""
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    (m1, a1), (m2, a2) = _op_model(), _op_model()
    guard = StepGuard(**guard_kw)
    o1 = FusedSGDAdam(m1, a1, consts[0], momentum=0.9, weight_decay=1e-3).use_device_schedule(*consts).use_step_guard(guard)
    o2 = FusedSGDAdam(m2, a2, consts[0], momentum=0.9, weight_decay=1e-3).use_device_schedule(*consts)
    return (m1, a1, o1, guard), (m2, a2, o2)


def _compare(m1, o1, m2, o2):
    """SGD parameters and momentum buffers torch.equal; Adam's tensors to the project's 2e-6 bar.  Returns whether Adam's are equal."""
    n_sgd = n_adam = 0
    adam_equal = True
    for (k, p1, b1, adam), (_, p2, b2, _) in zip(_sgd_adam_split(m1, o1), _sgd_adam_split(m2, o2)):
        if adam:
            n_adam += 1
            d = float((p1 - p2).detach().abs().max()) / (1e-6 + float(p2.detach().abs().max()))
            assert d <= 2e-6, (k, d)
            adam_equal = adam_equal and torch.equal(p1, p2) and torch.equal(b1, b2)
        else:
            n_sgd += 1
            assert torch.equal(p1, p2), k
            assert torch.equal(b1, b2), k
    assert n_sgd > 100 and n_adam > 10
    return adam_equal


def test_idle_guard_equals_the_unguarded_optimiser():
    """max_norm=None, finite gradients, three steps: clip_coef is exactly 1 and 1 * g is g, the schedule is one shared function."""
    (m1, a1, o1, guard), (m2, a2, o2) = _pair(dict(max_norm=None))
    gen = torch.Generator(device=DEV).manual_seed(6)
    for it in range(3):
        g = torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1
        a1.flat.copy_(g)
        a2.flat.copy_(g)
        o1.step()
        o2.step()
    torch.cuda.synchronize()
    print("idle guard: Adam tensors equal:", _compare(m1, o1, m2, o2))
    assert o1.iteration() == 3 and o2.iteration() == 3
    assert torch.equal(o1.last_lr(), o2.last_lr())
    rec = guard.read()
    assert list(rec["t"]) == [0, 1, 2] and not rec["skipped"].any() and not rec["clipped"].any() and rec["dropped"] == 0
    assert (rec["clip_coef"] == 1.0).all() and (rec["nonfinite"] == 0).all()
    assert torch.equal(a1.flat, g)                                # the arena is read, never written


def test_clipping_against_torch():
    """Three steps against CPU clip_grad_norm_ + torch.optim.SGD / Adam, driven like test_device_schedule_vs_torch_optim (its
    metric, its 2e-6 bar).  Gradient scales 0.1, 0.05, 0.01 and max_norm = 0.03 sqrt(N): steps 0 and 1 clip, step 2 does not.
    clip_coef is held to one f32 ulp of the float64 rule at the float64 norm of the gradients (nothing the device computed enters
    the reference).  The device forms the coefficient from its norm in double and rounds once, so what it adds to that rounding's
    half ulp is half the relative error of its sum of squares; torch's own f32 coefficient is printed beside it."""
    from cavp_amd.optim import FusedSGDAdam, StepGuard, set_group_lr
    m, arena = _op_model()
    ref = {k: p.detach().cpu().clone().requires_grad_(True) for k, p in m.named_parameters()}
    names = {id(p): k for k, p in m.named_parameters()}
    lr0, mom, wd = SHORT[0], 0.9, 1e-3
    groups = [dict({kk: vv for kk, vv in g.items() if kk != "params"}, params=[ref[names[id(p)]] for p in g["params"]],
                   lr=g["lr"] * lr0) for g in set_group_lr(m, 1.0)]
    opt_v = torch.optim.SGD(groups, lr=lr0, momentum=mom, weight_decay=wd)
    opt_a = torch.optim.Adam([ref["audio_backbone." + k] for k, _ in m.audio_backbone.named_parameters()], lr=lr0)
    guard = StepGuard(max_norm=1.0)
    fused = FusedSGDAdam(m, arena, lr0, momentum=mom, weight_decay=wd).use_device_schedule(*SHORT).use_step_guard(guard)
    n_elems = sum(p.numel() for p in fused.params)
    max_norm = 0.03 * math.sqrt(n_elems)
    guard.set_max_norm(max_norm)
    never = {id(p) for p in m.params_without_grad()}
    clipped_params = [ref[names[id(p)]] for p in fused.params]
    gen = torch.Generator(device=DEV).manual_seed(5)
    last = guard.last()
    for it, scale in enumerate((0.1, 0.05, 0.01)):
        lr = host_lr(it, SHORT)
        arena.flat.copy_(torch.randn(arena.flat.numel(), generator=gen, device=DEV) * scale)
        raw = arena.flat.clone()
        for k, p in m.named_parameters():
            ref[k].grad = None if id(p) in never else arena.views[id(p)].detach().cpu().clone()
        # clip_grad_norm_ on float64 copies of the gradients: its f32 norm of these 115 M elements is itself off by 1.6e-3 on
        # the CPU (printed), a thousand times the bar, so the f32 call cannot referee a 2e-6 comparison
        doubles = [torch.zeros(1, dtype=torch.float64).expand(r.shape) for r in clipped_params]
        for d, r in zip(doubles, clipped_params):
            d.grad = r.grad.double()
        norm64 = float(torch.nn.utils.clip_grad_norm_(doubles, max_norm))
        total = float(torch.nn.utils.clip_grad_norm_(clipped_params, float("inf")))     # the f32 norm only: coefficient 1
        for d, r in zip(doubles, clipped_params):
            r.grad = d.grad.float()
        del doubles
        for i, g in enumerate(opt_v.param_groups):
            g["lr"] = lr * (1.0 if i < 4 else 10.0)
        opt_v.step()
        opt_a.step()
        fused.step()
        norm, coef = float(last["grad_norm"].item()), float(last["clip_coef"].item())
        worst = _worst(m, ref)
        torch_coef = min(1.0, max_norm / (total + 1e-6))
        print(f"step {it}: norm {norm:.9e} (float64 {norm64:.9e}, torch {total:.9e}), coef {coef:.9e} (torch {torch_coef:.9e}), "
              f"worst relative difference {worst:.3e}")
        assert abs(norm - norm64) <= 2e-6 * norm64
        assert within_one_ulp(coef, R.clip_coef(norm64, max_norm)), (it, coef, R.clip_coef(norm64, max_norm))
        assert (coef < 1.0) == (it < 2)
        assert worst <= 2e-6, (it, worst)
        assert torch.equal(arena.flat, raw)                        # p.grad keeps the raw gradient (torch scales it in place)
    rec = guard.read()
    assert list(rec["clipped"]) == [True, True, False] and not rec["skipped"].any() and list(rec["t"]) == [0, 1, 2]
    assert fused.iteration() == 3


def test_skip_then_recover():
    """clean, NaN-planted, clean: t ends at 2, skipped_total at 1, and the result is that of an unguarded optimiser that only saw
    the two clean gradients (equality classes of the idle test)."""
    (m1, a1, o1, guard), (m2, a2, o2) = _pair(dict(max_norm=None))
    gen = torch.Generator(device=DEV).manual_seed(7)
    for it in range(3):
        g = torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1
        a1.flat.copy_(g)
        if it == 1:
            a1.views[id(o1.params[5])].view(-1)[0] = float("nan")
        else:
            a2.flat.copy_(g)
            o2.step()
        o1.step()
    torch.cuda.synchronize()
    print("skip then recover: Adam tensors equal:", _compare(m1, o1, m2, o2))
    assert o1.iteration() == 2 and o2.iteration() == 2
    assert int(guard.last()["skipped_total"].item()) == 1
    rec = guard.read()
    assert list(rec["t"]) == [0, 1, 1] and list(rec["skipped"]) == [False, True, False] and list(rec["nonfinite"]) == [0, 1, 0]
    assert not rec["skipped_on_loss"].any()                         # a skip on a gradient is told apart from one on a loss
    sd = o1.state_dict()
    assert sd["guard"] == {"skipped_total": 1, "max_norm": None} and sd["t"] == 2
    assert "guard" not in o2.state_dict()
    # the checkpoint restores the guard's counter and bound; a dict without the entry (an unguarded optimiser's) still loads
    guard.set_max_norm(3.0)
    sd["guard"] = {"skipped_total": 5, "max_norm": None}
    o1.load_state_dict(sd)
    assert int(guard.last()["skipped_total"].item()) == 5 and guard.max_norm is None
    assert float(guard._view("max_norm", torch.float32).item()) == 0.0
    o1.load_state_dict(o2.state_dict())
    assert int(guard.last()["skipped_total"].item()) == 5 and o1.iteration() == 2


def test_skipped_first_step_keeps_first_step():
    """Step 0 skipped, then a clean step: it still runs as t = 0 with first_step set, i.e. the momentum buffer is overwritten, not
    decayed - visible because both momentum buffers start from ones here."""
    (m1, a1, o1, guard), (m2, a2, o2) = _pair(dict(max_norm=None))
    o1.state_m.fill_(1.0)
    o2.state_m.fill_(1.0)
    gen = torch.Generator(device=DEV).manual_seed(8)
    g = torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1
    a1.flat.copy_(g)
    a1.views[id(o1.params[0])].view(-1)[-1] = float("inf")
    o1.step()
    assert o1.iteration() == 0
    sgd = [(p, b) for _, p, b, adam in _sgd_adam_split(m1, o1) if not adam]
    assert all(bool((b == 1.0).all()) for _, b in sgd)
    a1.flat.copy_(g)
    a2.flat.copy_(g)
    o1.step()
    o2.step()
    torch.cuda.synchronize()
    for (k, p1, b1, adam), (_, p2, b2, _) in zip(_sgd_adam_split(m1, o1), _sgd_adam_split(m2, o2)):
        if not adam:
            assert torch.equal(p1, p2) and torch.equal(b1, b2), k
    assert o1.iteration() == 1
    rec = guard.read()
    assert list(rec["t"]) == [0, 0] and list(rec["skipped"]) == [True, False]


def test_ring_drops_the_oldest_records():
    """history = 4, six steps, the fourth with a NaN: read() returns the last four records with dropped == 2; a skipped step keeps
    its index and rate for the next one; a second read() returns nothing."""
    (m1, a1, o1, guard), _ = _pair(dict(max_norm=None, history=4), consts=SHORT)
    gen = torch.Generator(device=DEV).manual_seed(9)
    skips = [0, 0, 0, 1, 0, 0]
    loss = torch.zeros(1, device=DEV)
    for it, s in enumerate(skips):
        a1.flat.copy_(torch.randn(a1.flat.numel(), generator=gen, device=DEV) * 0.1)
        if s:
            a1.views[id(o1.params[3])].view(-1)[0] = float("nan")
        loss.fill_(10.0 + it)
        o1.step(losses=(loss,))
    want, (t_end, skipped_total) = R.record_sequence(skips, lambda t: host_lr(t, SHORT))
    idx, dropped = R.ring_read(len(skips), 4, 0)
    rec = guard.read()
    assert rec["dropped"] == dropped == 2
    assert list(rec["t"]) == [want[i][0] for i in idx] == [2, 3, 3, 4]
    assert list(rec["skipped"]) == [want[i][2] for i in idx]
    assert list(rec["l_ce"]) == [10.0 + i for i in idx]
    for got, i in zip(rec["lr"], idx):
        assert within_one_ulp(got, want[i][1]), (i, got, want[i][1])
    assert not rec["clipped"].any() and (rec["flags"] & 4 == 0).all() and (rec["flags"] & 8 != 0).all()
    assert o1.iteration() == t_end == 5 and int(guard.last()["skipped_total"].item()) == skipped_total == 1
    again = guard.read()
    assert len(again["t"]) == 0 and again["dropped"] == 0


# ------------------------------------------------------------------------------------------------------------ captured step
def test_captured_step_with_guard(deterministic):
    """CFG2, the update recorded with a guard: the records carry t = 0, 1, 2, the loss each replay returned (bit-equal) and the
    last_lr() sequence; the parameters equal those of a captured run without a guard (fixed-order mode, max_norm=None)."""
    from cavp_amd.optim import StepGuard
    m1, o1, (image, audio, label) = _with_optimizer(CFG2, seed=11)
    m2, o2, _ = _with_optimizer(CFG2, seed=11)
    guard = StepGuard(max_norm=None, history=8)
    o1.use_step_guard(guard)
    r1 = m1.capture_train_step(image, audio, label, optimizer=o1)
    r2 = m2.capture_train_step(image, audio, label, optimizer=o2)
    assert o1.iteration() == 0 and len(guard.read()["t"]) == 0     # the capture itself runs nothing
    sd = _state(m1)
    m2.load_state_dict(sd)
    losses, rates = [], []
    for it in range(3):
        losses.append(np.float32(r1().item()))
        rates.append(np.float32(o1.last_lr().item()))
        r2()
    torch.cuda.synchronize()
    rec = guard.read()
    print(f"captured with guard: losses {losses}, records {rec['l_ce']}, norms {rec['grad_norm']}")
    assert list(rec["t"]) == [0, 1, 2] and rec["dropped"] == 0
    assert rec["l_ce"].tobytes() == np.array(losses, dtype=np.float32).tobytes()
    assert rec["lr"].tobytes() == np.array(rates, dtype=np.float32).tobytes()
    for it, r in enumerate(rates):
        assert within_one_ulp(r, host_lr(it, CAP)), (it, r)
    assert not rec["skipped"].any() and (rec["grad_norm"] > 0).all() and np.isfinite(rec["grad_norm"]).all()
    assert (rec["flags"] & 4 == 0).all()
    a, b = _state(m1), _state(m2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(o1.state_m, o2.state_m) and torch.equal(o1.state_v, o2.state_v)
    assert any(not torch.equal(a[k], sd[k]) for k, _ in m1.named_parameters())


def test_captured_step_with_guard_and_contrast():
    """CFG3 with the contrast term on the device sampler: each record carries that replay's l_ce and l_ctr."""
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    from cavp_amd.synth import synth_inputs
    from tests.test_gpu_train_model import _build
    B = CFG3["B"]
    image, audio, label = synth_inputs(B, CFG3["hw"], audio_batch=2 * B, num_classes=3, seed=21)
    label[:, 8:40, 8:48] = 1
    label[:, 44:60, 4:60] = 2
    label[:, :4] = 255
    image, audio, label = image.to(DEV), audio.to(DEV), label.to(DEV)
    shuf = label.roll(1, 0).contiguous()
    m, _ = _build(CFG3)
    m.train_step(image, audio, label)
    guard = StepGuard(max_norm=None, history=8)
    opt = FusedSGDAdam(m, m._grad_arena, 1e-3, momentum=0.9, weight_decay=1e-4).use_device_schedule(*CAP).use_step_guard(guard)
    crit = ContrastLoss(temperature=0.1, ignore_idx=255, max_views=32).use_device_sampler(4, seed=1234)
    replay = m.capture_train_step(image, audio, label, contrast=crit, label_shuffle=shuf, optimizer=opt)
    ce, ctr = [], []
    for it in range(3):
        replay()
        ce.append(np.float32(m._last_losses[0].item()))
        ctr.append(np.float32(m._last_losses[1].item()))
    rec = guard.read()
    print(f"captured with guard + contrast: l_ce {rec['l_ce']}, l_ctr {rec['l_ctr']}")
    assert list(rec["t"]) == [0, 1, 2] and not rec["skipped"].any()
    assert rec["l_ce"].tobytes() == np.array(ce, dtype=np.float32).tobytes()
    assert rec["l_ctr"].tobytes() == np.array(ctr, dtype=np.float32).tobytes()
    assert (rec["l_ctr"] > 0).all() and (rec["flags"] & 12 == 0).all()
    assert opt.iteration() == 3


def test_loss_rule_is_refused_with_collectives_on(monkeypatch):
    """Data parallel the loss is this rank's own while the gradients are reduced: a guard whose loss rule is on is refused before
    anything is launched (collectives_on() is patched; no process group is needed to reach the check)."""
    import cavp_amd.train as TR
    from cavp_amd._lib import CavpError
    from cavp_amd.optim import StepGuard
    m, opt, (image, audio, label) = _with_optimizer(CFG2, seed=15)
    opt.use_step_guard(StepGuard())
    before = [p.detach().clone() for p in m.parameters()]
    stats = {k: b.clone() for k, b in m.named_buffers()}
    monkeypatch.setattr(TR, "collectives_on", lambda: True)
    with pytest.raises(CavpError, match="skip_nonfinite_loss=False"):
        m.capture_train_step(image, audio, label, optimizer=opt)
    torch.cuda.synchronize()
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), before))
    assert all(torch.equal(b, stats[k]) for k, b in m.named_buffers())
    assert opt.iteration() == 0 and len(opt._guard.read()["t"]) == 0


# --------------------------------------------------------------------------------------------------------------- end to end
def test_all_ignored_batch_is_skipped():
    """train_step on a batch whose labels are all 255, then step(losses=...).  The loss is NaN as torch's is; on this path the CE
    head gives that batch ZERO gradients (not NaN ones), so the gradients alone would let momentum and weight decay move the
    weights: the guard skips on the recorded loss.  NaN here is ordinary data - no address depends on a value."""
    from cavp_amd.optim import StepGuard
    m, opt, (image, audio, label) = _with_optimizer(CFG2, seed=14)
    guard = StepGuard(max_norm=1.0)
    opt.use_step_guard(guard)
    opt.step()                                                     # one ordinary step first: momentum is not zero any more
    assert opt.iteration() == 1
    ignored = torch.full_like(label, 255)
    want = torch.nn.functional.cross_entropy(torch.zeros(1, CFG2["C"], 2, 2), torch.full((1, 2, 2), 255), ignore_index=255)
    assert math.isnan(float(want))
    before = [p.detach().clone() for p in m.parameters()]
    m_before, v_before = opt.state_m.clone(), opt.state_v.clone()
    loss = m.train_step(image, audio, ignored)
    opt.step(losses=(loss,))
    torch.cuda.synchronize()
    assert math.isnan(float(loss.item()))
    assert int(guard.last()["skip"].item()) == 1
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), before))
    assert torch.equal(opt.state_m, m_before) and torch.equal(opt.state_v, v_before)
    assert opt.iteration() == 1
    rec = guard.read()
    assert list(rec["skipped"]) == [False, True] and list(rec["t"]) == [0, 1] and math.isnan(float(rec["l_ce"][1]))
    assert list(rec["skipped_on_loss"]) == [False, True] and int(rec["nonfinite"][1]) == 0
    print(f"all-ignored batch: gradient norm {rec['grad_norm'][1]:.3e}, non-finite gradient elements {rec['nonfinite'][1]}")
    # a clean batch afterwards trains again
    m.train_step(image, audio, label)
    opt.step()
    assert opt.iteration() == 2 and any(not torch.equal(p, b) for p, b in zip(m.parameters(), before))
