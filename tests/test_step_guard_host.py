"""Host side of the step guard: the float64 restatement of its rules against torch's clip_grad_norm_, the ctypes mirrors of
struct cavp_guard_state / cavp_step_record against the header and the library, the new prototypes, and the argument errors of
StepGuard / use_step_guard.  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _step_guard_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float}


# ------------------------------------------------------------------------------------------------------------- the rules
def _cpu_grads(seed, scale):
    g = torch.Generator().manual_seed(seed)
    shapes = [(1,), (3,), (5, 7), (4097,), (64, 33)]
    return [torch.randn(s, generator=g) * scale for s in shapes]


@pytest.mark.parametrize("max_norm, clipped", [(1.0, True), (1e4, False)], ids=["clipped", "unclipped"])
def test_reference_matches_torch_clip_grad_norm(max_norm, clipped):
    """torch computes the norm and the coefficient in f32: the norm agrees to f32 rounding of a 5-tensor stack (1e-6), the scaled
    gradients to a few f32 ulps."""
    grads = _cpu_grads(3, 0.5)
    params = [torch.zeros_like(g).requires_grad_(True) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    ref = R.guard_step([g.numpy() for g in grads], [0, 1, 0, 1, 0], max_norm=max_norm)
    assert abs(ref["grad_norm"] - total) <= 1e-6 * total
    assert (ref["clip_coef"] < 1.0) == clipped
    assert ref["nonfinite"] == 0 and not ref["skip"]
    assert abs(math.hypot(ref["norm_sgd"], ref["norm_adam"]) - ref["grad_norm"]) <= 1e-12 * ref["grad_norm"]
    for p, g in zip(params, grads):
        want = g.double() * ref["clip_coef"]
        assert float((p.grad.double() - want).abs().max()) <= 4e-7 * float(want.abs().max())
        if not clipped:
            assert torch.equal(p.grad, g)


def test_reference_skip_rule():
    g = [np.ones(5), np.ones(4097)]
    assert not R.guard_step(g, [0, 1])["skip"]
    for bad in (np.nan, np.inf, -np.inf):
        h = [g[0].copy(), g[1].copy()]
        h[1][-1] = bad
        r = R.guard_step(h, [0, 1], max_norm=1.0)
        assert r["nonfinite"] == 1 and r["skip"]
        assert not R.guard_step(h, [0, 1], skip_nonfinite=False)["skip"]
    big = R.guard_step([np.full(3, 3e19)], [0])          # finite, but the squares leave the f32 range
    assert big["nonfinite"] == 0 and math.isinf(big["grad_norm"]) and big["skip"]
    on_loss = R.guard_step(g, [0, 1], losses=(float("nan"),))
    assert on_loss["skip"] and on_loss["skip_on_loss"]
    assert R.guard_step(g, [0, 1], losses=(float("nan"),), skip_nonfinite=False)["skip"]          # two independent switches
    off = R.guard_step(g, [0, 1], losses=(float("nan"),), skip_nonfinite_loss=False)
    assert not off["skip"] and not off["skip_on_loss"]
    assert not R.guard_step(g, [0, 1], losses=(1.5, 0.0))["skip"]
    assert R.clip_coef(0.0, 2.0) == 1.0 and R.clip_coef(4.0, None) == 1.0 and R.clip_coef(4.0, 0.0) == 1.0
    assert R.clip_coef(4.0, 2.0) == 2.0 / (4.0 + 1e-6)


def test_reference_record_sequence_and_ring():
    recs, (t, skipped) = R.record_sequence([0, 0, 0, 1, 0, 0], lambda t: 10.0 - t)
    assert [r[0] for r in recs] == [0, 1, 2, 3, 3, 4] and (t, skipped) == (5, 1)
    assert recs[3] == (3, 7.0, True) and recs[4] == (3, 7.0, False)
    assert R.ring_read(6, 4, 0) == ([2, 3, 4, 5], 2)
    assert R.ring_read(6, 4, 6) == ([], 0)
    assert R.ring_read(3, 4, 1) == ([1, 2], 0)


# ------------------------------------------------------------------------------------------------------------ the mirrors
def _header_fields(struct):
    hdr = open(os.path.join(REPO, "include", "cavp_hip.h")).read()
    body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"\b(int64_t|int32_t|double|float)\s+([a-z0-9_]+)\s*;", body)


def test_guard_structs_match_header():
    """Same field names, order and C types as the header's structs."""
    from cavp_amd.optim import GuardState, StepRecord
    for struct, mirror in (("cavp_guard_state", GuardState), ("cavp_step_record", StepRecord)):
        fields = _header_fields(struct)
        assert [(n, C_TYPES[t]) for t, n in fields] == [(n, t) for n, t in mirror._fields_], struct
    for name in ("max_norm", "skip_nonfinite", "history", "grad_norm", "norm_sgd", "norm_adam", "nonfinite", "clip_coef", "skip",
                 "skipped_total", "head"):
        assert hasattr(GuardState, name), name
    for name in ("t", "l_ce", "l_ctr", "lr_sgd", "grad_norm", "clip_coef", "nonfinite", "flags"):
        assert hasattr(StepRecord, name), name
    # the 8-byte fields are naturally aligned, and the ring behind the state block starts on an 8-byte boundary
    for f in ("nonfinite", "skipped_total", "head"):
        assert getattr(GuardState, f).offset % 8 == 0
    assert ctypes.sizeof(GuardState) % 8 == 0 and ctypes.sizeof(StepRecord) % 8 == 0
    assert np.dtype(StepRecord).itemsize == ctypes.sizeof(StepRecord)


def test_guard_flags_match_header():
    from cavp_amd import optim
    hdr = open(os.path.join(REPO, "include", "cavp_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (CAVP_STEP_[A-Z0-9_]+) +(\d+)", hdr)}
    assert got == {"CAVP_STEP_SKIPPED": optim.STEP_SKIPPED, "CAVP_STEP_CLIPPED": optim.STEP_CLIPPED,
                   "CAVP_STEP_NO_LOSS": optim.STEP_NO_LOSS, "CAVP_STEP_NO_LOSS1": optim.STEP_NO_LOSS1,
                   "CAVP_STEP_SKIPPED_LOSS": optim.STEP_SKIPPED_LOSS}
    bits = {k: int(v) for k, v in re.findall(r"#define (CAVP_GUARD_SKIP_[A-Z]+) +(\d+)", hdr)}
    assert bits == {"CAVP_GUARD_SKIP_GRADIENTS": optim.GUARD_SKIP_GRADIENTS, "CAVP_GUARD_SKIP_LOSSES": optim.GUARD_SKIP_LOSSES}


def test_guard_struct_sizes_match_library():
    from cavp_amd import _lib, build
    from cavp_amd.optim import GuardState, StepRecord
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.cavp_guard_state_bytes() == ctypes.sizeof(GuardState)
    assert lib.cavp_step_record_bytes() == ctypes.sizeof(StepRecord)


def test_guard_prototypes_are_declared():
    from cavp_amd import _lib
    want = {"cavp_guard_state_bytes": 0, "cavp_step_record_bytes": 0, "cavp_grad_guard_partials": 5, "cavp_grad_guard_finish": 6,
            "cavp_optimizer_schedule_guarded": 5, "cavp_optimizer_step_guarded": 8}
    for name, nargs in want.items():
        assert name in _lib.PROTOTYPES, name
        assert len(_lib.PROTOTYPES[name][1]) == nargs, name
    # the guard is additive: the ABI number and the unguarded entry points are what they were
    assert _lib.ABI_VERSION == 16
    assert len(_lib.PROTOTYPES["cavp_optimizer_schedule"][1]) == 2 and len(_lib.PROTOTYPES["cavp_optimizer_step_dev"][1]) == 7


# ------------------------------------------------------------------------------------------------------------- the errors
def test_step_guard_argument_errors():
    from cavp_amd._lib import CavpError
    from cavp_amd.optim import StepGuard
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(CavpError):
            StepGuard(max_norm=bad)
    for bad in (0, -3, 1.5, None, True, (1 << 24) + 1):
        with pytest.raises(CavpError):
            StepGuard(history=bad)
    g = StepGuard(max_norm=2, skip_nonfinite=0, history=1)
    assert g.max_norm == 2.0 and g.skip_nonfinite is False and g.history == 1
    assert StepGuard().max_norm is None and StepGuard().history == 1024
    assert StepGuard().skip_nonfinite_loss is True and StepGuard(skip_nonfinite_loss=0).skip_nonfinite_loss is False
    for call in (g.read, g.last):                       # not attached yet: nothing to read
        with pytest.raises(CavpError):
            call()
    with pytest.raises(CavpError):
        g.set_max_norm(-1.0)
    g.set_max_norm(None)
    assert g.max_norm is None


class _Fake:
    """just enough of FusedSGDAdam for use_step_guard's checks, which come before any device work"""
    _sched = None
    _guard = None

    def _need_sched(self, what):
        from cavp_amd.optim import FusedSGDAdam
        return FusedSGDAdam._need_sched(self, what)


def test_use_step_guard_argument_errors():
    from cavp_amd._lib import CavpError
    from cavp_amd.optim import FusedSGDAdam, StepGuard
    fake = _Fake()
    with pytest.raises(CavpError):
        FusedSGDAdam.use_step_guard(fake, object())          # not a StepGuard
    with pytest.raises(CavpError):
        FusedSGDAdam.use_step_guard(fake, StepGuard())       # no device schedule
    with pytest.raises(CavpError):
        FusedSGDAdam.step(fake, losses=(torch.zeros(1),))    # losses without a guard
    assert fake._guard is None
