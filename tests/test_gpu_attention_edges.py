"""The three attention families against float64 (tests/_attn_ref.py) at the Nk / Nq / T / batch edges of their kernels and on
peaked inputs: SRA softmax attention forward + backward (csrc/pvt_ops.hip, pvt_train.hip), the attention gate (csrc/attn_gate.hip)
and the one-key collapse (csrc/attn_rank1.hip), each in f32 and bf16.

Every tensor handed to a kernel is a 16-byte-aligned slice of a larger buffer: input bands are NaN, output bands a bit pattern
that must survive the call; no output element may be non-finite.  Bars (derived or calibrated per case against float64, never
against the kernel): _attn_ref.ratios.  Each test prints err / bar per output (`RATIO ...` lines; the worst per kernel and dtype
are recorded in DESIGN.md).  test_attn_ref_host.py shows on the CPU that wrong evaluations miss these bars at these cases."""
import ctypes as C

import pytest
import torch

from tests import _attn_ref as R
from tests._banded import DEV, Banded

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
DT = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])


def _cpu(t):
    return t.detach().float().cpu()


def _report(kernel, case_id, dtype, r):
    for name, v in r.items():
        print(f"RATIO {kernel} {'f32' if dtype == F32 else 'bf16'} {case_id} {name} {v:.4f}")
    assert R.within(r), (kernel, case_id, r)


NAN = float("nan")


# ---- SRA softmax attention ----------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("case", R.sra_cases(), ids=lambda c: c[0])
def test_sra_attention_forward_backward(case, dtype):
    """B = 2, heads = 2 at every Nk edge of the 16-key MFMA blocks, the 32-key bf16 pairs and the 64-key backward blocks, plus two
    shapes with more than one query block per workgroup.  cavp_sra_blocks_per_wg (common.h) takes the smallest qpw <= 8 with
    ceil(ceil(Nq / 64) / qpw) * B * heads <= 512:
      (2, 8, 2117, 17): 34 blocks x 16 = 544 > 512, qpw = 2 -> 17 workgroups, the last one ends on a block of 5 queries;
      (1, 16, 4101, 5): 65 blocks x 16 = 1040, qpw = 2 -> 33 x 16 = 528 > 512, qpw = 3 -> 22 workgroups = 66 blocks: the last
                        workgroup breaks out of its qb loop at block 65."""
    from cavp_amd import _lib, ops, train_ops as T
    cid, fam, B, heads, Nq, Nk, seed = case
    (q, kv, dout), ref, cal, bound = R.sra_setup(case, dtype)
    bands = Banded()
    qd, kvd, dd = bands.inp(q, dtype), bands.inp(kv, dtype), bands.inp(dout, dtype)
    o = bands.out("o", q.shape, dtype, NAN)
    dq, dkv = bands.out("dq", q.shape, dtype, NAN), bands.out("dkv", kv.shape, F32, NAN)      # outputs, not accumulators
    ops.sra_attention(qd, kvd, o, heads, 0.125)
    T.sra_attention_bwd(qd, kvd, dd, dq, dkv, heads, 0.125)
    bands.check()
    got = {"o": _cpu(o), "dq": _cpu(dq), "dkv": _cpu(dkv)}
    _report("sra", cid, dtype, R.ratios(got, ref, cal, dtype, bound))
    if Nk in (65, 129):
        dkv_c = bands.out("dkv_c", kv.shape, dtype, NAN)      # dkv stored in the compute dtype: the f32 result rounded once
        T.sra_attention_bwd(qd, kvd, dd, dq, dkv_c, heads, 0.125)
        bands.check()
        assert torch.equal(dkv_c, dkv.to(dtype))
        _lib.set_deterministic(True, device=torch.device(DEV))
        try:
            a, b = bands.out("dkv_a", kv.shape, F32, NAN), bands.out("dkv_b", kv.shape, F32, NAN)
            T.sra_attention_bwd(qd, kvd, dd, dq, a, heads, 0.125)
            T.sra_attention_bwd(qd, kvd, dd, dq, b, heads, 0.125)
            bands.check()
            assert torch.equal(a, b)
            _report("sra_det", cid, dtype, R.ratios({"dq": _cpu(dq), "dkv": _cpu(a)}, ref, cal, dtype, names=("dq", "dkv")))
        finally:
            _lib.set_deterministic(False)


def test_sra_attention_forward_refuses_unsupported_shapes():
    from cavp_amd import _lib, ops
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = torch.zeros((1, 64, 128), dtype=BF, device=DEV)
    kv = torch.zeros((1, 257, 256), dtype=BF, device=DEV)
    o = torch.full_like(q, 3.0)
    bf = ops.dtype_code(BF)
    assert lib.cavp_sra_attention(bf, p(q), p(kv), p(o), 1, 64, 256, 2, 64, C.c_float(0.125), s) == 0
    torch.cuda.synchronize()
    o.fill_(3.0)
    for nk, hd in ((257, 64), (256, 32)):
        st = lib.cavp_sra_attention(bf, p(q), p(kv), p(o), 1, 64, nk, 128 // hd, hd, C.c_float(0.125), s)
        assert st != 0 and b"unsupported" in lib.cavp_error_string(st).lower(), (nk, hd, st)
    torch.cuda.synchronize()
    assert bool((o == 3.0).all())                             # refused before any launch
    with pytest.raises(_lib.CavpError):
        ops.sra_attention(q, kv, o, 2, 0.125)                 # Nk = 257
    with pytest.raises(_lib.CavpError):
        ops.sra_attention(q, kv[:, :64].contiguous(), o, 4, 0.125)      # head_dim = 32


# ---- attention gate ---------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("case", R.gate_cases(), ids=lambda c: c[0])
def test_attn_gate_forward_backward(case, dtype):
    """The 4-head kernels (one DPP row per head) and the generic ones (masked wave reductions) with q_batch = B, a divisor of B
    and 1; fewer token rows than waves; dattn given and absent; saturated gates; accumulating dk / dv; deterministic mode."""
    from cavp_amd import _lib, ops, train_ops as T
    cid, fam, heads, hd, Tn, B, qb, da, seed = case
    (q, k, v, dout, dattn), ref, cal = R.gate_setup(case, dtype)
    scale, Cc = hd ** -0.5, heads * hd
    bands = Banded()
    qd, kd, vd, dd, dad = bands.inp(q, dtype), bands.inp(k, dtype), bands.inp(v, dtype), bands.inp(dout, dtype), bands.inp(dattn, F32)
    o, attn = bands.out("o", (B, Tn, Cc), dtype, NAN), bands.out("attn", (B, heads, Tn), F32, NAN)
    dq = bands.out("dq", (B, Tn, Cc), dtype, NAN)
    dk, dv = bands.out("dk", (B, Cc), F32, 0.0), bands.out("dv", (B, Cc), F32, 0.0)
    ops.attn_gate(qd, kd, vd, o, attn, heads, scale)
    T.attn_gate_bwd(dd, qd, kd, vd, attn, dad, dq, dk, dv, heads, scale)
    bands.check()
    got = {"o": _cpu(o), "attn": _cpu(attn), "dq": _cpu(dq), "dk": _cpu(dk), "dv": _cpu(dv)}
    _report("gate", cid, dtype, R.ratios(got, ref, cal, dtype))
    # dk and dv accumulate: a second call gives twice the gradient
    T.attn_gate_bwd(dd, qd, kd, vd, attn, dad, dq, dk, dv, heads, scale)
    bands.check()
    twice = lambda d: {n: 2 * d[n] for n in ("dk", "dv")}
    _report("gate_twice", cid, dtype, R.ratios({"dk": _cpu(dk), "dv": _cpu(dv)}, twice(ref), twice(cal), dtype))
    _lib.set_deterministic(True, device=torch.device(DEV))
    try:
        runs = []
        for tag in "ab":
            dq2 = bands.out("dq_" + tag, (B, Tn, Cc), dtype, NAN)
            dk2, dv2 = bands.out("dk_" + tag, (B, Cc), F32, 0.0), bands.out("dv_" + tag, (B, Cc), F32, 0.0)
            T.attn_gate_bwd(dd, qd, kd, vd, attn, dad, dq2, dk2, dv2, heads, scale)
            runs.append((dq2, dk2, dv2))
        bands.check()
        assert all(torch.equal(x, y) for x, y in zip(*runs))
        _report("gate_det", cid, dtype, R.ratios(dict(zip(("dq", "dk", "dv"), map(_cpu, runs[0]))), ref, cal, dtype, names=("dq", "dk", "dv")))
    finally:
        _lib.set_deterministic(False)


# ---- one-key collapse -------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("case", R.rank1_cases(), ids=lambda c: c[0])
def test_attn_rank1_prepare_fwd_bwd_finish(case, dtype):
    """The smallest channel counts (d = 2, 4: the second row of attn1_finish's dk loop is always out of range), fewer token rows
    than waves, B = 9 and 16 (the 8-wide batch loops of attn1_finish and their tail), bp / dbp absent, saturated gates - against
    the float64 CPU evaluation.  (u, p, dU, dP, dk, dv and the workspace are allocated by the wrappers: a second pass through the
    C ABI puts bands around those as well.)"""
    from cavp_amd import ops, train_ops as T
    cid, fam, Cc, Tn, xb, reps, wb, wd, seed = case
    (x, k, v, wq, wp, bp, dout), ref, cal = R.rank1_setup(case, dtype)
    heads, B, scale = 4, xb * reps, (Cc // 4) ** -0.5
    bands = Banded()
    xd, kd, vd, dd = bands.inp(x, dtype), bands.inp(k, dtype), bands.inp(v, dtype), bands.inp(dout, dtype)
    wqd, wpd, bpd = bands.inp(wq, F32), bands.inp(wp, F32), bands.inp(bp, F32)
    assert ops.attn1_supported(Cc, heads)
    out, attn = bands.out("out", (B, Tn, Cc), dtype, NAN), bands.out("attn", (B, heads, Tn), F32, NAN)
    dx = bands.out("dx", (xb, Tn, Cc), dtype, NAN)
    dbp = bands.out("dbp", (Cc,), F32, 0.0) if wd else None
    dwq, dwp = bands.out("dwq", (Cc, Cc), F32, 0.0), bands.out("dwp", (Cc, Cc), F32, 0.0)
    u, pm = ops.attn1_prepare(wqd, wpd, kd, vd, heads, scale)
    ops.attn1_fwd(xd, u, pm, bpd, out, attn)
    du, dp = T.attn1_bwd(dd, xd, u, pm, dx, dbp)
    dk, dv = T.attn1_finish(wqd, wpd, kd, vd, du, dp, dwq, dwp, heads, scale)
    bands.check()
    assert all(bool(torch.isfinite(t).all()) for t in (u, pm, du, dp, dk, dv))
    got = {"out": _cpu(out), "attn": _cpu(attn), "dx": _cpu(dx), "dwq": _cpu(dwq), "dwp": _cpu(dwp), "dk": _cpu(dk), "dv": _cpu(dv)}
    if wd:
        got["dbp"] = _cpu(dbp)
    _report("rank1", cid, dtype, R.ratios(got, ref, cal, dtype, names=tuple(got)))
    # accumulate semantics of the parameter gradients (the flat arena is zeroed once per step, contributions add up)
    dk2, dv2 = T.attn1_finish(wqd, wpd, kd, vd, du, dp, dwq, dwp, heads, scale)
    bands.check()
    assert torch.equal(dk2, dk) and torch.equal(dv2, dv)
    twice = lambda d: {n: 2 * d[n] for n in ("dwq", "dwp")}
    _report("rank1_twice", cid, dtype, R.ratios({"dwq": _cpu(dwq), "dwp": _cpu(dwp)}, twice(ref), twice(cal), dtype))
    # the same four launches through the C ABI with the wrapper-allocated tensors banded too: same bits (every sum of this
    # family has a fixed order), bands intact
    from cavp_amd import _lib
    lib, code = _lib.load(), ops.dtype_code(dtype)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u2, pm2 = bands.out("u", (B, heads, Cc), F32, NAN), bands.out("pm", (B, heads, Cc), F32, NAN)
    du2, dp2 = bands.out("du", (B, heads, Cc), F32, NAN), bands.out("dp", (B, heads, Cc), F32, NAN)
    dk3, dv3 = bands.out("dk", (B, Cc), F32, NAN), bands.out("dv", (B, Cc), F32, NAN)
    out2, attn2 = bands.out("out2", (B, Tn, Cc), dtype, NAN), bands.out("attn2", (B, heads, Tn), F32, NAN)
    dx2 = bands.out("dx2", (xb, Tn, Cc), dtype, NAN)
    dbp2 = bands.out("dbp2", (Cc,), F32, 0.0) if wd else None
    dwq2, dwp2 = bands.out("dwq2", (Cc, Cc), F32, 0.0), bands.out("dwp2", (Cc, Cc), F32, 0.0)
    nbytes = lib.cavp_attn1_bwd_workspace_bytes(B, xb, Tn, Cc, heads)
    ws = bands.out("ws", (nbytes // 4,), F32, 0.0)
    assert lib.cavp_attn1_prepare(code, p(wqd), p(wpd), p(kd), p(vd), p(u2), p(pm2), B, Cc, heads, C.c_float(scale), s) == 0
    assert lib.cavp_attn1_fwd(code, p(xd), p(u2), p(pm2), p(bpd), p(out2), p(attn2), B, xb, Tn, Cc, heads, s) == 0
    assert lib.cavp_attn1_bwd(code, p(dd), p(xd), p(u2), p(pm2), p(dx2), p(du2), p(dp2), p(dbp2), p(ws), C.c_size_t(nbytes), B, xb, Tn, Cc,
                              heads, s) == 0
    assert lib.cavp_attn1_finish(code, p(wqd), p(wpd), p(kd), p(vd), p(du2), p(dp2), p(dwq2), p(dwp2), p(dk3), p(dv3), B, Cc, heads,
                                 C.c_float(scale), s) == 0
    bands.check()
    for name, a, b in (("u", u2, u), ("pm", pm2, pm), ("out", out2, out), ("attn", attn2, attn), ("dx", dx2, dx), ("du", du2, du),
                       ("dp", dp2, dp), ("dk", dk3, dk), ("dv", dv3, dv)):
        assert torch.equal(a, b), name
    assert dbp2 is None or torch.equal(dbp2, dbp)
    assert R.within(R.ratios({"dwq": _cpu(dwq2), "dwp": _cpu(dwp2)}, ref, cal, dtype, names=("dwq", "dwp")))
