"""Host side of the gradient accumulator (cavp_amd/accumulate.py, csrc/grad_accum.hip, the gated twins in csrc/optimizer.hip): the
numpy reference against torch's own .grad accumulation, the k / gate and loss-mean rules, the ctypes mirror and the prototypes
against the header and the library, and every refusal.  No GPU needed."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _accumulate_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cavp_accum_state_bytes": 0, "cavp_grad_accumulate": 7, "cavp_accum_advance": 4, "cavp_optimizer_schedule_gated": 3,
         "cavp_optimizer_step_dev_gated": 8, "cavp_grad_guard_partials_gated": 6, "cavp_grad_guard_finish_gated": 7,
         "cavp_optimizer_schedule_guarded_gated": 6, "cavp_optimizer_step_guarded_gated": 9}
UNGATED = {"cavp_optimizer_schedule_gated": "cavp_optimizer_schedule", "cavp_optimizer_step_dev_gated": "cavp_optimizer_step_dev",
           "cavp_grad_guard_partials_gated": "cavp_grad_guard_partials", "cavp_grad_guard_finish_gated": "cavp_grad_guard_finish",
           "cavp_optimizer_schedule_guarded_gated": "cavp_optimizer_schedule_guarded",
           "cavp_optimizer_step_guarded_gated": "cavp_optimizer_step_guarded"}
C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def _header():
    return open(os.path.join(REPO, "include", "cavp_hip.h")).read()


# ------------------------------------------------------------------------------------------------- the reference equals torch
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_reference_sum_equals_torch_grad_accumulation(n):
    """(loss / N).backward() N times on different inputs: p.grad is bit for bit the reference's sequential f32 sum of the per-call
    gradients (each taken alone from a zeroed .grad)."""
    torch.manual_seed(100 + n)
    net = nn.Sequential(nn.Linear(37, 19), nn.Tanh(), nn.Linear(19, 5)).float()
    xs = [torch.randn(11, 37) * (1.0 + i) for i in range(n)]
    ys = [torch.randn(11, 5) for _ in range(n)]
    singles = []
    for x, y in zip(xs, ys):
        net.zero_grad(set_to_none=True)
        (((net(x) - y) ** 2).mean() / n).backward()
        singles.append([p.grad.detach().clone().numpy() for p in net.parameters()])
    net.zero_grad(set_to_none=True)
    for x, y in zip(xs, ys):
        (((net(x) - y) ** 2).mean() / n).backward()
    for j, p in enumerate(net.parameters()):
        want = R.window_sum([s[j] for s in singles])
        assert want.dtype == np.float32 and p.grad.numpy().tobytes() == want.tobytes(), (n, j)
    if n == 1:
        assert R.window_sum([singles[0][0]]).tobytes() == singles[0][0].tobytes()


# ----------------------------------------------------------------------------------------------------------- k, gate, means
def test_gate_and_k_sequences():
    assert R.gate_sequence(1, 7) == [(0, 1)] * 7
    assert R.gate_sequence(2, 7) == [(0, 0), (1, 1), (0, 0), (1, 1), (0, 0), (1, 1), (0, 0)]
    assert R.gate_sequence(3, 7) == [(0, 0), (1, 0), (2, 1), (0, 0), (1, 0), (2, 1), (0, 0)]
    assert R.gate_sequence(3, 2, k0=1) == [(1, 0), (2, 1)]                 # a run resumed inside a window
    recs, end = R.record_sequence(3, [False] * 2 + [True] + [False] * 4, lambda t: 0.1 * (t + 1))
    assert recs == [(2, 0, 0.1, True), (5, 0, 0.1, False)] and end == (1, 1, 2, 1)   # the skipped window leaves t alone
    recs, end = R.record_sequence(1, [False, True, False], lambda t: float(t))
    assert [r[1] for r in recs] == [0, 1, 1] and end == (2, 1, 3, 0)


def test_loss_means_follow_the_rule():
    """N = 3 is no power of two: the quotient is rounded.  The reference's mean is the correctly rounded f32 quotient of the
    sequential f32 sum (checked against exact rational arithmetic), and forming it in float64 first gives the same bits - the
    kernel's route."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    for trial in range(2000):
        losses = (rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        s = np.float32(np.float32(losses[0] + losses[1]) + losses[2])
        assert R.loss_sum(losses).tobytes() == s.tobytes()
        mean = R.window_mean(losses)
        assert mean.tobytes() == R.window_mean_via_float64(losses).tobytes()
        exact = Fraction(float(s)) / 3
        lo, hi = np.nextafter(mean, np.float32(-np.inf)), np.nextafter(mean, np.float32(np.inf))
        err = abs(Fraction(float(mean)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (trial, losses)
    assert R.window_mean([np.float32(1.0)] * 3) == np.float32(1.0)
    assert np.isnan(R.window_mean([np.float32(1.0), np.float32(np.nan), np.float32(2.0)]))
    assert R.window_mean([np.float32(0.25)]).tobytes() == np.float32(0.25).tobytes()


# ------------------------------------------------------------------------------------------------------------ the boundary
def test_state_struct_matches_header_and_library():
    from cavp_amd import _lib, build
    from cavp_amd.accumulate import AccumState
    build.build(verbose=False)
    hdr = _header()
    body = hdr[hdr.index("typedef struct cavp_accum_state {"):hdr.index("} cavp_accum_state;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|int32_t|float)\s+([a-z0-9_]+)\s*;", body)
    assert [(n, C_TYPES[t]) for t, n in fields] == [(n, t) for n, t in AccumState._fields_]
    assert _lib.load().cavp_accum_state_bytes() == ctypes.sizeof(AccumState) == 48
    assert AccumState.gate.offset == 8 and AccumState.loss_mean0.offset == 40


def test_prototypes_header_and_exports_agree():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert hasattr(raw, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl is not None, name
        params = [p for p in decl.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == nargs, (name, params)
    for gated, plain in UNGATED.items():       # a twin is its original plus the gate word, in front of the stream
        assert _lib.PROTOTYPES[gated][1] == _lib.PROTOTYPES[plain][1][:-1] + [ctypes.c_void_p] + _lib.PROTOTYPES[plain][1][-1:]
    assert "cavp_optimizer_step_gated" not in _lib.PROTOTYPES    # the host-scalar step has no twin
    assert _lib.ABI_VERSION == 16 and _lib.load().cavp_abi_version() == 16
    assert int(re.search(r"#define CAVP_ABI_VERSION (\d+)", hdr).group(1)) == 16
    declared = set(re.findall(r"\b(cavp_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(_lib.PROTOTYPES)
    assert "grad_accum.hip" in build.SOURCES


# ------------------------------------------------------------------------------------------------------------ the refusals
def _cpu_optimizer(sched=True):
    """A FusedSGDAdam shell over a CPU arena: the fields the accumulator's constructor reads, no launch is ever issued."""
    from cavp_amd.optim import FusedSGDAdam
    flat = torch.zeros(64)
    p = torch.zeros(8)
    opt = FusedSGDAdam.__new__(FusedSGDAdam)
    opt._arena = types.SimpleNamespace(flat=flat, views={id(p): flat[16:24]})
    opt.params = [p]
    opt._sched = torch.zeros(96, dtype=torch.uint8) if sched else None
    opt._guard = None
    return opt


def test_constructor_refusals():
    from cavp_amd._lib import CavpError
    from cavp_amd.accumulate import GradAccumulator
    with pytest.raises(CavpError, match="FusedSGDAdam"):
        GradAccumulator(object(), 2)
    for bad in (0, -1, True, 2.0, None, (1 << 16) + 1):
        with pytest.raises(CavpError, match="micro_steps"):
            GradAccumulator(_cpu_optimizer(), bad)
    with pytest.raises(CavpError, match="device schedule"):
        GradAccumulator(_cpu_optimizer(sched=False), 2)
    opt = _cpu_optimizer()
    acc = GradAccumulator(opt, 3)
    assert acc.flat.shape == opt._arena.flat.shape and acc.flat.dtype == torch.float32 and acc.nbytes == 4 * 64
    assert acc.read() == {"k": 0, "windows": 0, "micro_total": 0, "window_losses": (0.0, 0.0)}
    with pytest.raises(CavpError, match="already has an accumulator"):
        GradAccumulator(opt, 3)
    outside = _cpu_optimizer()
    outside._arena.views[id(outside.params[0])] = torch.zeros(8)
    with pytest.raises(CavpError, match="outside its arena"):
        GradAccumulator(outside, 2)
    with pytest.raises(CavpError, match="no StepGuard"):
        acc.step(losses=(torch.zeros(1),))
    sd = acc.state_dict()
    assert sd["k"] == 0 and sd["micro_steps"] == 3 and torch.equal(sd["acc"], acc.flat)
    other = GradAccumulator(_cpu_optimizer(), 2)
    with pytest.raises(CavpError, match="micro_steps"):
        other.load_state_dict(sd)
    sd["k"] = 2
    acc.load_state_dict(sd)
    assert acc.read()["k"] == 2
    acc.reset()
    assert acc.read()["k"] == 0


def test_capture_refusals(monkeypatch):
    """capture_train_step(accumulate=): no optimiser, a foreign optimiser, rollback=, collectives on - refused before any launch
    (collectives_on() is patched; no process group is needed to reach the check)."""
    import cavp_amd.train as TR
    from cavp_amd._lib import CavpError
    from cavp_amd.accumulate import GradAccumulator
    from cavp_amd.cavp_model import CAVP
    x = torch.zeros(1)
    opt = _cpu_optimizer()
    acc = GradAccumulator(opt, 2)

    def call(**kw):
        return CAVP.capture_train_step(types.SimpleNamespace(), x, x, x, **kw)
    with pytest.raises(CavpError, match="GradAccumulator"):
        call(optimizer=opt, accumulate=object())
    with pytest.raises(CavpError, match="needs optimizer="):
        call(accumulate=acc)
    with pytest.raises(CavpError, match="another optimiser"):
        call(optimizer=_cpu_optimizer(), accumulate=acc)
    with pytest.raises(CavpError, match="rollback="):
        call(optimizer=opt, accumulate=acc, rollback=object())
    monkeypatch.setattr(TR, "collectives_on", lambda: True)
    with pytest.raises(CavpError, match="collectives on"):
        call(optimizer=opt, accumulate=acc)
