"""Gradient accumulation on the GPU (cavp_amd/accumulate.py; cavp_grad_accumulate / cavp_accum_advance and the gated twins of the
optimiser's launches).  Kernel level on the hand-built job table of test_gpu_step_guard.py: window equality against torch's f32
sum and an ungated twin, the accumulator and the padding, a non-finite window, the loss means, the launch count.  Model level
on CFG2: a captured window against an eager twin, with and without a guard, and the default route beside the new kwarg."""
import types

import numpy as np
import pytest
import torch

from cavp_amd.synth import synth_inputs
from tests import _accumulate_ref as R
from tests.test_gpu_optim_sched import CFG2, _state, _with_optimizer
from tests.test_gpu_step_guard import Table, _fields, _guard, _sched, _sched_fields

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0


# ------------------------------------------------------------------------------------------------------- hand-built job table
def _table_opt(tab, guard_kw=None):
    """A FusedSGDAdam over a hand-built table (no model): the fields step() and the accumulator read."""
    from cavp_amd.optim import FusedSGDAdam
    opt = FusedSGDAdam.__new__(FusedSGDAdam)
    opt._arena = types.SimpleNamespace(flat=tab.arena, views={id(p): g for p, g in zip(tab.p, tab.g)})
    opt.params, opt.table, opt.njobs, opt.total_blocks = tab.p, tab.table, tab.njobs, tab.total_blocks
    opt.momentum, opt.eps, opt._steps, opt.state_m = 0.9, 1e-8, 0, tab.arena
    opt._model = lambda: None
    opt._sched = _sched(0)
    opt._guard = _guard(tab, **guard_kw) if guard_kw is not None else None
    return opt


def _mask(tab):
    """True where an arena float belongs to a gradient view, False on the padding between views"""
    mask = torch.zeros(tab.arena.numel(), dtype=torch.bool)
    for g in tab.g:
        o = (g.data_ptr() - tab.arena.data_ptr()) // 4
        mask[o:o + g.numel()] = True
    assert 0 < int((~mask).sum()) < 64
    return mask


def _pmv(tab):
    return [t.clone() for ts in (tab.p, tab.m, tab.v) for t in ts]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _torch_sum(grads):
    """torch-CPU sequential f32 sum, the order of .grad accumulation"""
    s = grads[0].clone()
    for g in grads[1:]:
        s = s + g
    return s


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_window_equality(n, guarded):
    """Two windows of n micro-steps with fresh random gradients before each.  A micro-step that does not close its window leaves
    parameters, m, v, the arena, the schedule block and the whole guard buffer (ring included) byte-equal; a closing one leaves
    the torch-CPU sequential f32 sum in the arena (the padding untouched) and parameters, state, schedule and guard equal to a
    twin table that received that sum and one ungated step()."""
    from cavp_amd.accumulate import GradAccumulator
    kw = dict(max_norm=0.5, history=4) if guarded else None
    ta, tb = Table(seed=3), Table(seed=3)
    oa, ob = _table_opt(ta, kw), _table_opt(tb, kw)
    acc = GradAccumulator(oa, n)
    mask = _mask(ta)
    gen = torch.Generator(device=DEV).manual_seed(40 + n)
    la, lb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    closed = 0
    for w in range(2):
        grads, losses = [], []
        for k in range(n):
            g = torch.randn(ta.arena.numel(), generator=gen, device=DEV) * 0.1
            ta.arena.copy_(g)
            grads.append(g.cpu())
            losses.append(np.float32(0.3 + 0.37 * k + w))
            la.fill_(float(losses[-1]))
            before = _pmv(ta), oa._sched.clone(), (oa._guard._buf.clone() if guarded else None)
            acc.step(losses=(la,) if guarded else None)
            torch.cuda.synchronize()
            if k < n - 1:
                assert _same(_pmv(ta), before[0]) and torch.equal(oa._sched, before[1]), (w, k)
                assert torch.equal(ta.arena, g), (w, k)
                assert not guarded or torch.equal(oa._guard._buf, before[2]), (w, k)
                assert acc.read()["k"] == k + 1
                continue
            closed += 1
            want = _torch_sum(grads)
            assert want.numpy().tobytes() == R.window_sum([x.numpy() for x in grads]).tobytes()
            got = ta.arena.cpu()
            assert got[mask].numpy().tobytes() == want[mask].numpy().tobytes(), (w, n)
            assert torch.equal(got[~mask], grads[-1][~mask])                      # the padding is never written
            if n == 1:
                assert torch.equal(ta.arena, g)                                    # nothing to sum: the arena is left alone
            tb.arena.copy_(want.to(DEV))
            lb.fill_(float(R.window_mean(losses)))
            ob.step(losses=(lb,) if guarded else None)
            torch.cuda.synchronize()
            assert _same(_pmv(ta), _pmv(tb)), (w, n)
            assert not _same(_pmv(ta), before[0])
            assert torch.equal(oa._sched, ob._sched) and _sched_fields(oa._sched).t == closed
            if guarded:
                assert torch.equal(oa._guard._buf, ob._guard._buf)
                assert _fields(oa._guard).head == closed and _fields(oa._guard).clip_coef < 1.0
            rd = acc.read()
            assert (rd["k"], rd["windows"], rd["micro_total"]) == (0, closed, closed * n)


def test_accumulator_and_padding():
    """n = 3: after k = 0 the accumulator is a byte copy of the arena on every view, after k = 1 the f32 sum, and the closing
    micro-step does not write it; the padding floats between views keep their sentinel in the accumulator and in the arena."""
    from cavp_amd.accumulate import GradAccumulator
    tab = Table(seed=5)
    opt = _table_opt(tab)
    acc = GradAccumulator(opt, 3)
    mask = _mask(tab)
    acc.flat.fill_(SENTINEL)
    gen = torch.Generator(device=DEV).manual_seed(77)
    grads = []
    for k in range(3):
        g = torch.randn(tab.arena.numel(), generator=gen, device=DEV)
        g[~mask.to(DEV)] = SENTINEL
        tab.arena.copy_(g)
        grads.append(g.cpu())
        held = acc.flat.clone()
        acc.step()
        torch.cuda.synchronize()
        a = acc.flat.cpu()
        assert bool((a[~mask] == SENTINEL).all()) and bool((tab.arena.cpu()[~mask] == SENTINEL).all()), k
        if k == 0:
            assert a[mask].numpy().tobytes() == grads[0][mask].numpy().tobytes()
        elif k == 1:
            assert a[mask].numpy().tobytes() == (grads[0] + grads[1])[mask].numpy().tobytes()
        else:
            assert torch.equal(acc.flat, held)
            assert tab.arena.cpu()[mask].numpy().tobytes() == _torch_sum(grads)[mask].numpy().tobytes()


def test_nonfinite_window_is_skipped_and_does_not_leak():
    """An inf in micro-step 0 of a 3-step window: one record, flagged skipped, skipped_total + 1, t unchanged, nothing updated.
    The next, clean window updates and equals a twin that only ever saw the clean window: k = 0 copies, so the poison stays
    behind the boundary."""
    from cavp_amd.accumulate import GradAccumulator
    ta, tb = Table(seed=9), Table(seed=9)
    oa, ob = _table_opt(ta, dict(max_norm=None, history=4)), _table_opt(tb, dict(max_norm=None, history=4))
    acc = GradAccumulator(oa, 3)
    mask = _mask(ta).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(13)
    start = _pmv(ta)
    for k in range(3):
        g = torch.randn(ta.arena.numel(), generator=gen, device=DEV) * 0.1
        if k == 0:   # element 4098 of the long unaligned view: scalar path, second block
            g[(ta.g[-2].data_ptr() - ta.arena.data_ptr()) // 4 + 4098] = float("inf")
        ta.arena.copy_(g)
        acc.step()
    torch.cuda.synchronize()
    rec = oa._guard.read()
    assert list(rec["t"]) == [0] and list(rec["skipped"]) == [True] and rec["nonfinite"][0] >= 1
    assert _fields(oa._guard).skipped_total == 1 and _sched_fields(oa._sched).t == 0
    assert _same(_pmv(ta), start)
    clean = []
    for k in range(3):
        g = torch.randn(ta.arena.numel(), generator=gen, device=DEV) * 0.1
        ta.arena.copy_(g)
        clean.append(g.cpu())
        acc.step()
        if k == 0:
            assert bool(torch.isfinite(acc.flat[mask]).all())
    tb.arena.copy_(_torch_sum(clean).to(DEV))
    ob.step()
    torch.cuda.synchronize()
    assert _same(_pmv(ta), _pmv(tb)) and not _same(_pmv(ta), start)
    assert torch.equal(oa._sched, ob._sched) and _sched_fields(oa._sched).t == 1
    rec = oa._guard.read()
    assert list(rec["t"]) == [0] and list(rec["skipped"]) == [False]
    fa, fb = _fields(oa._guard), _fields(ob._guard)
    assert (fa.skipped_total, fa.head, fa.skip) == (1, 2, 0) and np.float32(fa.grad_norm).tobytes() == np.float32(fb.grad_norm).tobytes()
    assert acc.read()["windows"] == 2


def test_loss_means():
    """n = 3, two loss words, two windows: the guard's record and acc.read() carry the reference's window means byte for byte.
    Observed: exact - the kernel forms sum / 3 in double and rounds once more, which is the correctly rounded f32 quotient, so
    the one-ulp allowance for a division that is not correctly rounded is not needed and not granted."""
    from cavp_amd.accumulate import GradAccumulator
    tab = Table(seed=2)
    opt = _table_opt(tab, dict(max_norm=None, history=4))
    acc = GradAccumulator(opt, 3)
    rng = np.random.default_rng(8)
    l0, l1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    want = []
    for w in range(2):
        ce = (rng.random(3) * 3.0 + 0.1).astype(np.float32)
        ctr = (rng.random(3) * 7.0 + 0.1).astype(np.float32)
        for k in range(3):
            l0.copy_(torch.from_numpy(ce[k:k + 1]))
            l1.copy_(torch.from_numpy(ctr[k:k + 1]))
            acc.step(losses=(l0, l1))
        want.append((R.window_mean(ce), R.window_mean(ctr)))
    rec = opt._guard.read()
    print(f"window means: records {rec['l_ce']} {rec['l_ctr']}, reference {want} - observed exact (correctly rounded)")
    assert len(rec["t"]) == 2 and (rec["flags"] & 12 == 0).all()
    assert rec["l_ce"].tobytes() == np.array([w[0] for w in want], dtype=np.float32).tobytes()
    assert rec["l_ctr"].tobytes() == np.array([w[1] for w in want], dtype=np.float32).tobytes()
    got = acc.read()["window_losses"]
    assert np.float32(got[0]).tobytes() == want[1][0].tobytes() and np.float32(got[1]).tobytes() == want[1][1].tobytes()


def test_launch_count():
    """A micro-step issues at most two launches more than the same step without accumulation: the accumulate launch and the
    state advance, then one gated twin per launch of step() (two unguarded, four guarded), in step()'s order."""
    from cavp_amd.accumulate import GradAccumulator
    plain = {False: ["cavp_optimizer_schedule", "cavp_optimizer_step_dev"],
             True: ["cavp_grad_guard_partials", "cavp_grad_guard_finish", "cavp_optimizer_schedule_guarded",
                    "cavp_optimizer_step_guarded"]}
    for guarded in (False, True):
        acc = GradAccumulator(_table_opt(Table(seed=1), dict(max_norm=None) if guarded else None), 4)
        names = acc.launch_names()
        assert names[:2] == ["cavp_grad_accumulate", "cavp_accum_advance"]
        assert [x[:-len("_gated")] for x in names[2:]] == plain[guarded] and all(x.endswith("_gated") for x in names[2:])
        assert len(names) - len(plain[guarded]) <= 2


# ------------------------------------------------------------------------------------------------------------- model level
SEEDS = (31, 32, 33, 34)
_RUNS = {}


def _batches():
    B = CFG2["B"]
    return [[t.to(DEV) for t in synth_inputs(B, CFG2["hw"], audio_batch=2 * B, num_classes=CFG2["C"], seed=s)] for s in SEEDS]


def _captured_run(guarded):
    """Capture with accumulate=GradAccumulator(opt, 2), then four replays on four different batches.  Shared by the tests below
    (computed once per flavour, inside a test that holds the `deterministic` fixture)."""
    if guarded in _RUNS:
        return _RUNS[guarded]
    from cavp_amd.accumulate import GradAccumulator
    from cavp_amd.optim import StepGuard
    m, opt, (image, audio, label) = _with_optimizer(CFG2, seed=11)
    guard = StepGuard(max_norm=None, history=8) if guarded else None
    if guarded:
        opt.use_step_guard(guard)
    acc = GradAccumulator(opt, 2)
    before = [p.detach().clone() for p in m.parameters()]
    replay = m.capture_train_step(image, audio, label, optimizer=opt, accumulate=acc)
    torch.cuda.synchronize()
    out = dict(after_capture=acc.read(), t_after_capture=opt.iteration(), init=_state(m),
               untouched=all(torch.equal(p, b) for p, b in zip(m.parameters(), before)), states=[], losses=[], m=[], v=[])
    for b in _batches():
        for dst, src in zip((image, audio, label), b):
            dst.copy_(src)
        out["losses"].append(np.float32(replay().item()))
        out["states"].append(_state(m))
        out["m"].append(opt.state_m.clone())
        out["v"].append(opt.state_v.clone())
    out.update(t=opt.iteration(), read=acc.read(), records=guard.read() if guarded else None,
               grad_is_arena=all(p.grad is None or p.grad.data_ptr() == m._grad_arena.views[id(p)].data_ptr()
                                 for p in m.parameters()))
    _RUNS[guarded] = out
    return out


def test_captured_window_against_eager_twin(deterministic):
    """Four replays = two windows of two.  The twin runs, per window, two eager train_step(loss_scale=0.5) with the arena cloned
    after each, writes g0 + g1 into the arena with torch and calls step(): state_dict (BatchNorm statistics included: two
    momentum updates per window on both sides), state_m and state_v are bit-equal after each closing replay; after a replay
    that closes nothing the parameters are the previous window's; t counts windows; the capture itself runs nothing."""
    run = _captured_run(False)
    assert run["after_capture"] == {"k": 0, "windows": 0, "micro_total": 0, "window_losses": (0.0, 0.0)}
    assert run["t_after_capture"] == 0 and run["untouched"]
    m2, o2, _ = _with_optimizer(CFG2, seed=11)
    m2.load_state_dict(run["init"])
    names = [k for k, _ in m2.named_parameters()]
    prev, gs = run["init"], []
    for i, (image, audio, label) in enumerate(_batches()):
        loss = m2.train_step(image, audio, label, loss_scale=0.5)
        gs.append(m2._grad_arena.flat.clone())
        assert np.float32(loss.item()).tobytes() == run["losses"][i].tobytes(), i     # the micro-step's loss, unscaled
        if i % 2 == 0:
            for k in names:
                assert torch.equal(run["states"][i][k], prev[k]), (i, k)
            continue
        m2._grad_arena.flat.copy_(gs[0] + gs[1])
        o2.step()
        torch.cuda.synchronize()
        twin = _state(m2)
        for k in twin:
            assert torch.equal(run["states"][i][k], twin[k]), (i, k)
        assert torch.equal(run["m"][i], o2.state_m) and torch.equal(run["v"][i], o2.state_v), i
        assert any(not torch.equal(twin[k], prev[k]) for k in names)
        prev, gs = twin, []
    assert run["t"] == 2 and o2.iteration() == 2 and run["grad_is_arena"]
    assert (run["read"]["k"], run["read"]["windows"], run["read"]["micro_total"]) == (0, 2, 4)


def test_captured_window_with_guard(deterministic):
    """The same run with StepGuard(max_norm=None, history=8): exactly two records, t = [0, 1], l_ce the reference mean of the
    window's two replay losses, parameters bit-equal to the unguarded accumulating run."""
    plain, run = _captured_run(False), _captured_run(True)
    assert run["after_capture"]["k"] == 0 and run["after_capture"]["windows"] == 0 and run["t_after_capture"] == 0
    rec = run["records"]
    print(f"accumulating with guard: losses {run['losses']}, records {rec['l_ce']}, norms {rec['grad_norm']}")
    assert list(rec["t"]) == [0, 1] and rec["dropped"] == 0 and not rec["skipped"].any()
    want = [R.window_mean(run["losses"][0:2]), R.window_mean(run["losses"][2:4])]
    assert rec["l_ce"].tobytes() == np.array(want, dtype=np.float32).tobytes()
    assert (rec["flags"] & 4 == 0).all() and (rec["grad_norm"] > 0).all() and np.isfinite(rec["grad_norm"]).all()
    assert [x.tobytes() for x in run["losses"]] == [x.tobytes() for x in plain["losses"]]
    for k in plain["states"][-1]:
        assert torch.equal(run["states"][-1][k], plain["states"][-1][k]), k
    assert torch.equal(run["m"][-1], plain["m"][-1]) and torch.equal(run["v"][-1], plain["v"][-1])
    assert run["t"] == 2


def test_default_route_untouched(deterministic):
    """optimizer= without accumulate=: one captured replay equals eager train_step + step() bit for bit, as before the kwarg."""
    m1, o1, (image, audio, label) = _with_optimizer(CFG2, seed=11)
    m2, o2, _ = _with_optimizer(CFG2, seed=11)
    replay = m1.capture_train_step(image, audio, label, optimizer=o1)
    assert getattr(o1, "_accum", None) is None
    m2.load_state_dict(_state(m1))
    l1 = np.float32(replay().item())
    l2 = np.float32(m2.train_step(image, audio, label).item())
    o2.step()
    torch.cuda.synchronize()
    a, b = _state(m1), _state(m2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(o1.state_m, o2.state_m) and torch.equal(o1.state_v, o2.state_v) and l1.tobytes() == l2.tobytes()
    assert o1.iteration() == 1 and o2.iteration() == 1
