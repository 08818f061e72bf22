"""The float64 BatchNorm references, the input families and the cases of test_gpu_bn_parity.py have teeth (CPU only): the explicit
formulas against torch.autograd of F.batch_norm in double, the tile combine against the direct statistics, the launch predicates
restated in _bn_ref against the case lists (every branch is reached in each dtype), the promises of the input families (no mask
ties, constant channels, the cancellation of the offset family) and - for every GPU case, in both dtypes - deliberately wrong
float64 evaluations that must land outside the bar the GPU test holds the kernel to."""
import pytest
import torch
import torch.nn.functional as F

from tests import _bn_ref as R

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
DT = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
SHAPE = {F32: R.shape_cases(F32), BF: R.shape_cases(BF)}
TILE = R.tile_cases()


def _rand(*shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ---- the formulas -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,act,with_res", [(2, 8, R.ACT_NONE, False), (5, 8, R.ACT_RELU, True), (65, 16, R.ACT_LEAKY, True),
                                                 (130, 24, R.ACT_RELU, False)])
def test_explicit_formulas_are_the_autograd_of_batch_norm(rows, C, act, with_res):
    z, dy, res = _rand(rows, C, seed=1) * 0.8 + 0.3, _rand(rows, C, seed=2), (_rand(rows, C, seed=3) if with_res else None)
    gamma, beta = _rand(C, seed=4).abs() + 0.5, _rand(C, seed=5)
    rm, rv = _rand(C, seed=6) * 0.1, _rand(C, seed=7).abs() + 0.5
    zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(zr, rm_t, rv_t, gr, br, True, R.MOM, R.EPS)
    y = y + res if with_res else y
    y = {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_LEAKY: lambda t: F.leaky_relu(t, R.SLOPE)}[act](y)
    y.backward(dy)
    got = R.chain_eval(z, dy, res, gamma, beta, act, 4)
    for name, ref in (("y_chain", y.detach()), ("dz_chain", zr.grad), ("dbeta", br.grad), ("dgamma", gr.grad)):
        assert R.rel_err(got[name], ref) <= 1e-12, name
    assert R.rel_err(R.bn_forward(z, gamma, beta, res, act), y.detach()) <= 1e-13
    # the finalize values, the running update with the unbiased variance included - by both statistics routes and the tile combine
    for mean, var in (R.stats_direct(z, None)[:2], R.stats_direct(z, z[0])[:2], R.stats_centred(z)[:2],
                      R.chan(R.tile_table(z, 3)[0], rows, 3)[:2]):
        v, _ = R.finish(mean, var, 0 * mean, 0 * var, gamma, beta, rows, rm, rv)
        assert R.rel_err(v["running_mean"], rm_t) <= 1e-12 and R.rel_err(v["running_var"], rv_t) <= 1e-12
        assert R.rel_err(z * v["scale"] + v["shift"], F.batch_norm(z, None, None, gamma, beta, True, R.MOM, R.EPS)) <= 1e-12
    swapped, _ = R.finish(mean, var, 0 * mean, 0 * var, gamma, beta, rows, rm, rv, mutant="swap_unbias")
    assert R.rel_err(swapped["running_var"], rv_t) > 1e-3 / rows


def test_apply_launch_formulas_are_the_chain_split_at_the_sums():
    """shape_eval's y / dz / sums (scale, shift, mean, rstd, sum_g, sum_gz as inputs) compose to the chain"""
    case = next(c for c in R.shape_cases(F32) if c.act == R.ACT_LEAKY and c.residual and c.family == "plain" and c.rows >= 63)
    inp, ref, _, _ = R.shape_setup(case, F32)
    ch = R.chain_eval(inp["z"], inp["dy"], inp["res"], inp["gamma"], inp["beta"], case.act, 4)
    assert R.rel_err(ref["y"], ch["y_chain"]) <= 1e-6           # (f32-rounded coefficients and y)
    assert R.rel_err(ref["sum_g"] - R.SUM0, ch["dbeta"]) <= 1e-5 and R.rel_err(ref["sum_gz"] - R.SUMSQ0, ch["dgamma"]) <= 1e-5
    assert R.rel_err(ref["dz"], ch["dz_chain"]) <= 1e-5


# ---- the case lists -------------------------------------------------------------------------------------------------------------------
@DT
def test_every_launch_branch_is_reached(dtype):
    cases = SHAPE[dtype]
    hit = set().union(*(R.branches(c, dtype) for c in cases))
    assert hit >= R.BRANCHES[dtype], R.BRANCHES[dtype] - hit
    v = R.ve(dtype)
    # the predicates at the widths of the table
    assert [R.flat_ok(C, dtype) for C in (8, 32, 48, 64, 72, 136, 256, 2048)] == [True, True, False, True, False, False, True, dtype == BF]
    assert R.flat_ok(1024, F32) and 1024 // 4 == 256 and 2048 // 8 == 256
    assert [R.reduce_groups(C, dtype) for C in (32, 48, 64, 72)] == ([8, 16, 16, 16] if dtype == F32 else [8, 8, 8, 16])
    assert R.reduce_groups(8 * v, dtype) == 8 and R.reduce_groups(8 * v + v, dtype) == 16
    assert {(c.C, c.ld) for c in cases} == set(R.W_NARROW + R.W_WIDE) - ({(1024, None)} if dtype == BF else set())
    for C, ld in R.W_NARROW:
        assert {c.rows for c in cases if c.C == C and c.rows <= 257} == set(R.ROWS_NARROW)
    assert {(c.C, c.rows) for c in cases if c.rows > 257} == {(C, r) for C in (8, 64) for r in R.ROWS_LONG}
    assert {c.rows for c in cases if c.C >= 256} == set(R.ROWS_WIDE)
    assert {c.family for c in cases} == set(R.FAMILIES) and {c.act for c in cases} == {0, 1, 2}
    for f in ("residual", "from_z", "g_out", "acc", "track"):
        assert {getattr(c, f) for c in cases} == {True, False}, f
    assert sum(c.det for c in cases) == 2
    assert {(c.act, c.residual, c.from_z) for c in cases} >= {(a, r, fz) for a in (1, 2) for r, fz in ((True, False), (False, True), (False, False))}
    assert all(c.rows * (c.ld or c.C) <= 4 << 20 for c in cases)
    assert {m for c in cases for m in R.shape_mutants(c, dtype)} == R.ALL_SHAPE_MUTANTS
    # about 300 GPU items: shape cases + tile cases in two dtypes, the wide tables once, chains, deterministic runs
    assert len(SHAPE[F32]) + len(SHAPE[BF]) + 2 * len(TILE) + 2 * 2 * len(R.CHAIN_WIDTHS) <= 320


def test_tile_cases_cover_both_finalize_kernels_and_the_fused_limit():
    from cavp_amd import train_ops as T
    assert R.BN_FUSED_TILES == T.BN_FUSED_TILES and R.BN_FUSED_TILES < 1024
    tiles = {c.tiles for c in TILE}
    assert tiles == {1, 2, 63, 64, 65, R.BN_FUSED_TILES, R.BN_FUSED_TILES + 1, 1023, 1024, 1025, 2051}
    assert {R.wide_finalize(t) for t in tiles} == {True, False} and {R.fused_route(t) for t in tiles} == {True, False}
    assert not R.wide_finalize(1023) and R.wide_finalize(1024) and R.fused_route(196) and not R.fused_route(197)
    assert all(c.rows == c.tiles * 8 - 3 and {cc.C for cc in TILE if cc.tiles == c.tiles} == {8, 72} for c in TILE)
    assert {c.world for c in TILE if R.wide_finalize(c.tiles)} == {1, 2, 8} and {c.track for c in TILE} == {True, False}
    assert {c.family for c in TILE if 2 <= c.tiles <= R.BN_FUSED_TILES} == set(R.FAMILIES)     # the fused launches meet every family
    assert {m for c in TILE for m in R.tile_mutants(c)} == {"ragged_full", "drop_last_tile", "swap_unbias"}


# ---- what the input families promise ---------------------------------------------------------------------------------------------------
@DT
def test_no_mask_tie_remains_in_any_case(dtype):
    n = 0
    for case in SHAPE[dtype]:
        if case.from_z:
            inp = R.shape_inputs(case, dtype)
            assert not bool(R.tie_mask(inp["z"], inp["scale"], inp["shift"]).any()), case.id
            n += 1
    assert n >= 8


@DT
def test_constant_channels_and_single_rows(dtype):
    seen = 0
    for case in SHAPE[dtype]:
        if case.family != "const" and case.rows != 1:
            continue
        inp, ref, _, _ = R.shape_setup(case, dtype)
        ch = slice(0, None, 4) if case.family == "const" else slice(None)
        z = inp["z"].double()
        assert bool((z[:, ch] == z[0, ch]).all())
        for route in ("fin_", "til_"):
            assert bool((ref[route + "rstd"][ch] == R.EPS ** -0.5).all()) and bool((ref[route + "mean"][ch] == z[0, ch]).all())
            if case.track and case.rows == 1:      # the `unbias` guard: M = 1 updates with the (zero) biased variance
                assert bool((ref[route + "running_var"] == (1 - R.MOM) * inp["rv0"].double()).all())
        assert all(bool(torch.isfinite(t).all()) for k, t in ref.items())
        seen += 1
    assert seen >= 20


@DT
def test_offset_family_cancels_in_the_unshifted_sums(dtype):
    """sum x^2 / M - mean^2 in f32 loses the variance of the offset family (which is why colstats runs it with a shift)"""
    case = next(c for c in SHAPE[dtype] if c.family == "offset" and c.rows == 257)
    inp, ref, _, _ = R.shape_setup(case, dtype)
    z = inp["z"]
    naive = (z * z).mean(0) - z.mean(0) ** 2
    var = ref["fin_rstd"] ** -2 - R.EPS
    assert float(((naive.double() - var).abs() / var).max()) > 1e-4
    assert inp["stat_shift"] is not None and abs(float(z.mean()) - 30.0) < 0.2


# ---- mutants: for every GPU case, wrong float64 evaluations miss that case's bar -------------------------------------------------------
def _missed(mut, ref, cal, bounds, dtype):
    r = R.ratios(mut, ref, cal, bounds, dtype)
    return not R.within(r), r


def _ids(c):
    return c.id


@pytest.mark.parametrize("case", SHAPE[F32], ids=_ids)
def test_shape_mutants_miss_the_bar_f32(case):
    _shape_mutants(case, F32)


@pytest.mark.parametrize("case", SHAPE[BF], ids=_ids)
def test_shape_mutants_miss_the_bar_bf16(case):
    _shape_mutants(case, BF)


def _shape_mutants(case, dtype):
    inp, ref, cal, bounds = R.shape_setup(case, dtype)
    again = R.shape_eval(inp, case, dtype)
    assert R.within(R.ratios(again, ref, cal, bounds, dtype))                    # the reference itself passes
    for m in R.shape_mutants(case, dtype):
        hit, r = _missed(R.shape_eval(inp, case, dtype, mutant=m), ref, cal, bounds, dtype)
        assert hit, (m, r)


@DT
@pytest.mark.parametrize("case", TILE, ids=_ids)
def test_tile_mutants_miss_the_bar(case, dtype):
    inp, ref, cal, bounds = R.tile_setup(case, dtype)
    assert R.within(R.ratios(R.tile_eval(inp, case, dtype), ref, cal, bounds, dtype))
    for m in R.tile_mutants(case):
        hit, r = _missed(R.tile_eval(inp, case, dtype, mutant=m), ref, cal, bounds, dtype)
        assert hit, (m, r)
