"""The BatchNorm training launches against float64 (tests/_bn_ref.py) on every launch route: the flat and the generic apply kernels,
the 8- and 16-group reduces, the one-wave and the wide tile combine, the moments of a rank and the second stage, the launches that
combine tile tables inside the apply pass - in f32 and bf16, at the row counts around the 16-row loop, the unrolled reduce trips and
the 64-row minimum block, on the plain, offset and constant-channel families and on M = 1.

Every tensor handed to a kernel is a slice of a guard-banded buffer (tests/_banded.py): NaN bands and NaN in the unused columns of
inputs, a bit pattern around outputs that must survive.  Each backward launch is tested on host-made inputs (y from the float64
forward, sums from float64), so a forward fault cannot cancel in a backward test; the chain tests run the launches end to end.
Bars (derived, or calibrated per case against float64 - never against the kernel): _bn_ref.ratios.  Each test prints err / bar per
output (`RATIO <kernel> <dtype> <case> <output> <err/bar>`; the worst per kernel are recorded in DESIGN.md 3b).
test_bn_ref_host.py shows on the CPU that wrong evaluations miss these bars at these cases."""
import pytest
import torch

from tests import _bn_ref as R
from tests._banded import DEV, Banded

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
NAN = float("nan")
FIN = ("mean", "rstd", "scale", "shift", "running_mean", "running_var")


def _cpu(t):
    return t.detach().float().cpu()


def _report(kernel, case_id, dtype, got, ref, cal, bounds, prefix=""):
    """got: {output name: device tensor}; compared with ref[prefix + name]"""
    g = {prefix + n: _cpu(t) for n, t in got.items() if t is not None}
    r = R.ratios(g, ref, cal, bounds, dtype)
    for name, v in r.items():
        print(f"RATIO {kernel} {'f32' if dtype == F32 else 'bf16'} {case_id} {name} {v:.4f}")
    assert R.within(r), (kernel, case_id, r)


def _vecs(bands, inp, names):
    return [bands.inp(inp[n], F32) for n in names]


def _fin_outs(bands, tag, C, inp):
    """NaN-filled scale / shift / mean / rstd and the running buffers holding their start values (or None)"""
    o = {n: bands.out(tag + n, (C,), F32, NAN) for n in FIN[:4]}
    for n, k in (("running_mean", "rm0"), ("running_var", "rv0")):
        o[n] = None
        if inp[k] is not None:
            o[n] = bands.out(tag + n, (C,), F32, 0.0)
            o[n].copy_(inp[k])
    return o


def _ids(c):
    return c.id


def _shape_params():
    return [pytest.param(c, dt, id=f"{c.id}-{'f32' if dt == F32 else 'bf16'}") for dt in (F32, BF) for c in R.shape_cases(dt)]


@pytest.mark.parametrize("case,dtype", _shape_params())
def test_launches_of_one_shape(case, dtype):
    """colstats (adding into non-zero buffers) -> bn_finalize; col_tile_stats -> bn_finalize_tiles; scale_shift_act with coefficients
    and without (the reshaping route, dense cases); bn_act_bwd_reduce (mask from y, or from z with the folded coefficients);
    bn_act_bwd_apply with g_out / acc as the case has them."""
    from cavp_amd import train_ops as T
    inp, ref, cal, bounds = R.shape_setup(case, dtype)
    rows, C, ld, c0 = case.rows, case.C, case.ld, case.col0
    B = Banded()
    zd, dyd, resd, yd = (B.inp_cols(inp[n], dtype, ld, c0) for n in ("z", "dy", "res", "y"))
    gamma, beta, mean, rstd, scale, shift, sum_g, sum_gz, shd = _vecs(B, inp, ("gamma", "beta", "mean", "rstd", "scale", "shift", "sum_g",
                                                                                "sum_gz", "stat_shift"))
    # forward statistics, shifted-sums route
    s, q = B.out("sum", (C,), F32, R.SUM0), B.out("sumsq", (C,), F32, R.SUMSQ0)
    T.colstats(zd, s, q, shd)
    s0, q0 = B.out("sum0", (C,), F32, 0.0), B.out("sumsq0", (C,), F32, 0.0)
    T.colstats(zd, s0, q0, shd)
    f = _fin_outs(B, "fin_", C, inp)
    T.bn_finalize(s0, q0, rows, gamma, beta, R.EPS, R.MOM, f["running_mean"], f["running_var"], f["scale"], f["shift"], f["mean"], f["rstd"],
                  stat_shift=shd)
    # forward statistics, tile route
    ts, tiles, rpt = T.col_tile_stats(zd)
    assert rpt == R.TILE_ROWS and tiles == -(-rows // rpt)
    t = _fin_outs(B, "til_", C, inp)
    T.bn_finalize_tiles(ts, tiles, rpt, rows, gamma, beta, R.EPS, R.MOM, t["running_mean"], t["running_var"], t["scale"], t["shift"], t["mean"],
                        t["rstd"])
    # forward apply
    y = B.out_cols("y", rows, C, dtype, NAN, ld, c0)
    T.scale_shift_act(zd, scale, shift, y, case.act, residual=resd)
    y0 = None
    if ld is None:
        y0 = B.out_cols("y0", rows, C, dtype, NAN)
        T.scale_shift_act(zd, None, None, y0, case.act, residual=resd)
    # backward reduce and apply on host-made inputs
    sg, sgz = B.out("sum_g", (C,), F32, R.SUM0), B.out("sum_gz", (C,), F32, R.SUMSQ0)
    fz = dict(fwd_scale=scale, fwd_shift=shift) if case.from_z else {}
    T.bn_act_bwd_reduce(dyd, None if case.from_z else yd, zd, mean, rstd, case.act, sg, sgz, **fz)
    dz = B.out_cols("dz", rows, C, dtype, NAN, ld, c0)
    g_out = B.out_cols("g", rows, C, dtype, NAN, ld, c0) if case.g_out else None
    acc = None
    if case.acc:
        acc = (B.out("dbeta", (C,), F32, 0.0), B.out("dgamma", (C,), F32, 0.0))
        acc[0].copy_(inp["acc0"][0])
        acc[1].copy_(inp["acc0"][1])
    T.bn_act_bwd_apply(dyd, None if case.from_z else yd, zd, mean, rstd, gamma, sum_g, sum_gz, case.act, dz, g_out=g_out, acc=acc, **fz)
    B.check()
    assert bool(torch.isfinite(ts).all())
    a = (ref, cal, bounds)
    _report("colstats", case.id, dtype, {"sum": s, "sumsq": q}, *a)
    _report("bn_finalize", case.id, dtype, f, *a, prefix="fin_")
    # the table's M2 about the tile means the launch stored (see _bn_ref.tile_table); its means against float64
    tref, tb = R.tile_table(inp["z"], R.TILE_ROWS, about=_cpu(ts)[..., 0])
    assert torch.equal(tref[..., 0], ref["table"][..., 0])
    tb[..., 0] = bounds["table"][..., 0]
    _report("col_tile_stats", case.id, dtype, {"table": ts}, dict(ref, table=tref), cal, dict(bounds, table=tb))
    _report("bn_finalize_tiles", case.id, dtype, t, *a, prefix="til_")
    _report("scale_shift_act", case.id, dtype, {"y": y, "y0": y0}, *a)
    _report("bn_act_bwd_reduce", case.id, dtype, {"sum_g": sg, "sum_gz": sgz}, *a)
    _report("bn_act_bwd_apply", case.id, dtype, {"dz": dz, "g": g_out, "dbeta": acc and acc[0], "dgamma": acc and acc[1]}, *a)


@pytest.mark.parametrize("case,dtype", [p for p in _shape_params() if p.values[0].det])
def test_reduces_in_deterministic_mode(case, dtype, deterministic):
    """fixed-order reductions: two runs agree bit for bit and both are within the bars"""
    from cavp_amd import train_ops as T
    inp, ref, cal, bounds = R.shape_setup(case, dtype)
    C = case.C
    B = Banded()
    zd, dyd, yd = (B.inp_cols(inp[n], dtype, case.ld, case.col0) for n in ("z", "dy", "y"))
    mean, rstd, scale, shift, shd = _vecs(B, inp, ("mean", "rstd", "scale", "shift", "stat_shift"))
    fz = dict(fwd_scale=scale, fwd_shift=shift) if case.from_z else {}
    runs = []
    for tag in "ab":
        o = {n: B.out(n + tag, (C,), F32, v) for n, v in (("sum", R.SUM0), ("sumsq", R.SUMSQ0), ("sum_g", R.SUM0), ("sum_gz", R.SUMSQ0))}
        T.colstats(zd, o["sum"], o["sumsq"], shd)
        T.bn_act_bwd_reduce(dyd, None if case.from_z else yd, zd, mean, rstd, case.act, o["sum_g"], o["sum_gz"], **fz)
        runs.append(o)
    B.check()
    assert all(torch.equal(runs[0][n], runs[1][n]) for n in runs[0])
    _report("reduces_det", case.id, dtype, runs[0], ref, cal, bounds)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", R.tile_cases(), ids=_ids)
def test_tile_tables(case, dtype, monkeypatch):
    """Host-made float64 (mean, M2) and (sum g, sum g zhat) tables cast to f32, 8 rows per tile, the last tile ragged: bn_finalize_tiles
    (one wave below 1024 tiles, the wide kernel from 1024), bn_tiles_to_moments and the second stage over `world` ranks,
    bn_bwd_sum_tiles (adding into non-zero buffers), and the two launches that combine the tables inside the apply pass (the wrappers
    fall back to two launches above the fused-tile limit: counted).  The fused backward's sum buffers are ZERO on entry, as its
    contract demands - also where it falls back to bn_bwd_sum_tiles, whose adding is checked by the separate call."""
    from cavp_amd import train_ops as T
    assert T.BN_FUSED_TILES == R.BN_FUSED_TILES
    inp, ref, cal, bounds = R.tile_setup(case, dtype)
    rows, C, tiles, rpt = case.rows, case.C, case.tiles, case.rpt
    B = Banded()
    zd, dyd, resd = (B.inp_cols(inp[n], dtype) for n in ("z", "dy", "res"))
    gamma, beta, mean, rstd, table, part, gathered = _vecs(B, inp, ("gamma", "beta", "mean", "rstd", "table", "part", "gathered"))
    f = _fin_outs(B, "fin_", C, inp)
    T.bn_finalize_tiles(table, tiles, rpt, rows, gamma, beta, R.EPS, R.MOM, f["running_mean"], f["running_var"], f["scale"], f["shift"],
                        f["mean"], f["rstd"])
    mom = B.out("moments", (C, 2), F32, NAN)
    T.bn_tiles_to_moments(table, tiles, rpt, rows, mom)
    s2 = _fin_outs(B, "st2_", C, inp)
    T.bn_finalize_tiles(gathered, case.world, rows, rows * case.world, gamma, beta, R.EPS, R.MOM, s2["running_mean"], s2["running_var"],
                        s2["scale"], s2["shift"], s2["mean"], s2["rstd"])
    sg, sgz = B.out("sum_g", (C,), F32, R.SUM0), B.out("sum_gz", (C,), F32, R.SUMSQ0)
    T.bn_bwd_sum_tiles(part, tiles, sg, sgz)
    # the fused launches (or, above the limit, the wrappers' two launches)
    fallbacks = []
    o_fin, o_sum = T._bn_finalize_tiles, T._bn_bwd_sum_tiles
    monkeypatch.setattr(T, "_bn_finalize_tiles", lambda *a: (fallbacks.append("fwd"), o_fin(*a))[1])
    monkeypatch.setattr(T, "_bn_bwd_sum_tiles", lambda *a: (fallbacks.append("bwd"), o_sum(*a))[1])
    u = _fin_outs(B, "fused_", C, inp)
    y = B.out_cols("y_fused", rows, C, dtype, NAN)
    T.scale_shift_act(zd, u["scale"], u["shift"], y, case.act, residual=resd,
                      bn_tiles=(table, tiles, rpt, gamma, beta, R.EPS, R.MOM, u["running_mean"], u["running_var"], u["mean"], u["rstd"]))
    fg, fgz = B.out("fsum_g", (C,), F32, 0.0), B.out("fsum_gz", (C,), F32, 0.0)
    dz = B.out_cols("dz_fused", rows, C, dtype, NAN)
    T.bn_act_bwd_apply(dyd, None, zd, mean, rstd, gamma, fg, fgz, R.ACT_NONE, dz, tile_partials=(part, tiles))
    B.check()
    assert fallbacks == ([] if R.fused_route(tiles) else ["fwd", "bwd"])
    a = (ref, cal, bounds)
    kernel = "bn_finalize_tiles_wide" if R.wide_finalize(tiles) else "bn_finalize_tiles"
    _report(kernel, case.id, dtype, f, *a)
    _report("bn_tiles_to_moments", case.id, dtype, {"moments": mom}, *a)
    _report("bn_finalize_tiles_stage2", case.id, dtype, s2, *a, prefix="st2_")
    _report("bn_bwd_sum_tiles", case.id, dtype, {"sum_g": sg, "sum_gz": sgz}, *a)
    _report("bn_tiles_scale_shift_act", case.id, dtype, dict(u, y_fused=y), *a)
    _report("bn_tiles_bwd_apply", case.id, dtype, {"dz_fused": dz, "fsum_g": fg, "fsum_gz": fgz}, *a)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("route", ["sums", "tiles"])
@pytest.mark.parametrize("width", R.CHAIN_WIDTHS, ids=lambda w: w[2])
def test_chain_against_float64_batch_norm(width, route, dtype):
    """z -> statistics -> apply and dy -> reduce -> apply, every launch fed by the launch before it, against float64 BatchNorm + ReLU
    forward and backward (130 rows: two tiles, the second ragged).  route "sums": colstats -> bn_finalize -> scale_shift_act;
    "tiles": col_tile_stats -> the apply launch that combines the table itself."""
    from cavp_amd import train_ops as T
    C, ld, _ = width
    rows, c0 = 130, 8 if ld else 0
    inp, ref, cal, bounds = R.chain_setup(C, rows, dtype, 9000 + C)
    B = Banded()
    zd, dyd = B.inp_cols(inp["z"], dtype, ld, c0), B.inp_cols(inp["dy"], dtype, ld, c0)
    gamma, beta = _vecs(B, inp, ("gamma", "beta"))
    scale, shift, mean, rstd = (B.out(n, (C,), F32, NAN) for n in ("scale", "shift", "mean", "rstd"))
    y = B.out_cols("y", rows, C, dtype, NAN, ld, c0)
    if route == "sums":
        s, q = B.out("sum", (C,), F32, 0.0), B.out("sumsq", (C,), F32, 0.0)
        T.colstats(zd, s, q)
        T.bn_finalize(s, q, rows, gamma, beta, R.EPS, R.MOM, None, None, scale, shift, mean, rstd)
        T.scale_shift_act(zd, scale, shift, y, R.ACT_RELU)
    else:
        ts, tiles, rpt = T.col_tile_stats(zd)
        T.scale_shift_act(zd, scale, shift, y, R.ACT_RELU, bn_tiles=(ts, tiles, rpt, gamma, beta, R.EPS, R.MOM, None, None, mean, rstd))
    sg, sgz = B.out("sum_g", (C,), F32, 0.0), B.out("sum_gz", (C,), F32, 0.0)
    T.bn_act_bwd_reduce(dyd, y, zd, mean, rstd, R.ACT_RELU, sg, sgz)
    dz = B.out_cols("dz", rows, C, dtype, NAN, ld, c0)
    T.bn_act_bwd_apply(dyd, y, zd, mean, rstd, gamma, sg, sgz, R.ACT_RELU, dz)
    B.check()
    _report("chain_" + route, f"c{C}{'in' + str(ld) if ld else ''}-r{rows}", dtype, {"y_chain": y, "dz_chain": dz, "dbeta": sg, "dgamma": sgz},
            ref, cal, bounds)
