"""float64 references, rounding models, input families, mutants and the case lists of the BatchNorm training launches
(csrc/train_pointwise.hip: colstats, col_tile_stats, bn_finalize, bn_finalize_tiles, bn_tiles_to_moments, scale_shift_act,
bn_act_bwd_reduce, bn_act_bwd_apply, bn_bwd_sum_tiles and the two launches that combine tile tables inside the apply pass).
CPU only; shared by test_bn_ref_host.py (no GPU) and test_gpu_bn_parity.py.

Reference rule: a reference consumes exactly the tensors the launch consumes (the dtype-rounded z / dy / y / residual, the f32
per-channel vectors and tile tables), converted to float64, and evaluates the textbook formula:
  y = act(z * scale + shift + res)          (scale, shift inputs)      y = act(gamma (z - mu) rstd + beta + res)   (chains)
  g = dy * act'(y),  dbeta = sum g,  dgamma = sum g zhat,  dz = gamma rstd (g - sum g / M - zhat sum g zhat / M)
  biased variance for the normalisation, unbiased (M > 1) in the running update.

Every evaluation takes `model`: None is the reference (float64); "f32" the same formula in PyTorch's f32 CPU arithmetic; "bf16" f32
arithmetic with the output rounded to bf16 where the kernel stores it.  The models only calibrate the bars of the element-wise
outputs (y, dz, g): rel_err = max |got - ref| / max |ref|, f32 bar max(4 e32, 1e-6), bf16 bar 3 e_bf16.

Per-channel reductions and what is derived from them carry a DERIVED bound instead (`red_bound`): a sum of n float64 terms t_i
computed in f32 in any order is held to |got - ref| <= 2^-24 (sqrt(n) + 8) sum |t_i|.  sqrt(n) is the random-walk growth of
n roundings of half an ulp of the running sum (<= sum |t_i|), 8 covers the handful of roundings that do not average (the final
LDS tree, the atomics, a division by M).  A value computed from such sums by a few f32 operations (variance, rstd, scale, shift,
running statistics) gets the bound of its inputs times the float64 derivative (`finish`).
Deviations from that formula, each because the literal bound is 0 (or below one rounding) where the launch still rounds:
  - one 2^-24 of the value per f32 rounding of the LAST expression of a derived quantity, counted: rstd 3 (var + eps, sqrt, 1 / x),
    scale 1, shift 2 (product, difference), running_mean 2, running_var 3, the mean of the shifted-sums route 1 (dm + shift);
  - the variance of the shifted-sums route (colstats -> bn_finalize) takes the terms of the sum that route forms, (z - shift)^2 / M,
    and the bound of dm through d var / d dm = -2 dm - not the centred squares: with the first row as shift, sum d^2 / M = var + dm^2
    is up to ~5 x var, and that is the magnitude at which this route rounds by construction (the issue says so of the unshifted
    case).  The tile route and every Chan combine are held to the centred squares.  CPU f32 sums (pairwise / double accumulation) are NOT used to calibrate reductions: they
under-state the error of a lane-chain + block order."""
import math
from collections import namedtuple
from functools import lru_cache

import torch

from tests._attn_ref import BF, F32, F64, _arith, _rb, rel_err

U = 2.0 ** -24
EPS, MOM, SLOPE = 1e-5, 0.1, 0.01
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
BN_FUSED_TILES = 196            # train_ops.BN_FUSED_TILES (the GPU test asserts they agree)
TILE_ROWS = 128                 # rows per tile of col_tile_stats
SUM0, SUMSQ0 = 0.25, -0.5       # what the sum buffers hold on entry: the reduces ADD


# ---- the host-side launch predicates of csrc/train_pointwise.hip, restated ------------------------------------------------------
def ve(dtype):
    """elements of a 16-byte channel vector"""
    return 4 if dtype == F32 else 8


def flat_ok(C, dtype):
    """flat_ok(): CV = C / VE vectors per row with 256 % CV == 0 (the coefficient vectors of the tests are 16-byte aligned)"""
    cv = C // ve(dtype)
    return C % ve(dtype) == 0 and 1 <= cv <= 256 and 256 % cv == 0


def reduce_groups(C, dtype):
    """launch_col_reduce: 8 column groups x 32 row lanes up to 8 * VE channels, else 16 x 16"""
    return 8 if C <= 8 * ve(dtype) else 16


def reduce_geometry(rows, C, dtype):
    """(CG, RL, gy, gx, rows_per_block) of col_reduce_kernel"""
    cg = reduce_groups(C, dtype)
    gy = -(-C // (cg * ve(dtype)))
    gx = max(768 // gy, 1)
    rpb = max(-(-rows // gx), 64)
    rpb = (rpb + 31) // 32 * 32
    return cg, 256 // cg, gy, -(-rows // rpb), rpb


def apply_geometry(rows, C, dtype):
    """("flat", CV, rows per trip, gx, rows_per_block) or ("generic", column chunks, 16, gx, rows_per_block) of the apply kernels"""
    v = ve(dtype)
    if flat_ok(C, dtype):
        cv = C // v
        rpt = 256 // cv
        rpb = max(-(-((16 << 10) // (C * (16 // v))) // rpt) * rpt, rpt)
        while -(-rows // rpb) > (1 << 20):
            rpb *= 2
        return "flat", cv, rpt, -(-rows // rpb), rpb
    gy = -(-C // (16 * v))
    gx = max(4096 // gy, 1)
    rpb = max(-(-rows // gx), 32)
    rpb = (rpb + 15) // 16 * 16
    return "generic", gy, 16, -(-rows // rpb), rpb


def wide_finalize(tiles):
    return tiles >= 1024


def fused_route(tiles):
    return tiles <= BN_FUSED_TILES


def branches(case, dtype):
    """the code paths one shape case reaches, as names (test_bn_ref_host.py asserts that every name is hit in each dtype)"""
    out = set()
    kind, n, rpt, gx, rpb = apply_geometry(case.rows, case.C, dtype)
    if kind == "flat":
        out.add("flat")
        out.add({1: "flat-1vec", 2: "flat-2vec", 256: "flat-256vec"}.get(n, "flat"))
        if case.ld is not None:
            out.add("flat-ld")
        if case.rows % rpt:
            out.add("flat-ragged-trip")
    else:
        out.add("generic")
        if n > 1:
            out.add("generic-chunks")
        if case.C % (16 * ve(dtype)):
            out.add("generic-ragged-chunk")
        if n == 32:
            out.add("generic-32chunks")
        if case.rows % 16:
            out.add("generic-ragged-trip")
    if gx > 1:
        out.add("apply-blocks")
        if case.rows % rpb:
            out.add("apply-ragged-block")
    cg, rl, gy, rgx, rrpb = reduce_geometry(case.rows, case.C, dtype)
    out.add(f"reduce-cg{cg}")
    if cg == 8 and case.C == 8 * ve(dtype):
        out.add("reduce-cg8-boundary")
    last = case.rows - (rgx - 1) * rrpb
    for blk in ({rrpb, last} if rgx > 1 else {last}):
        if blk >= 3 * rl + 1:
            out.add("reduce-unrolled")            # at least one lane makes a 4-row trip
            if blk % (4 * rl):
                out.add("reduce-unrolled-tail")   # and single rows follow it
        else:
            out.add("reduce-no-unrolled")
    if rgx > 1:
        out.add("reduce-blocks")
        if case.rows % rrpb:
            out.add("reduce-ragged-block")
    if -(-case.C // 64) > 1 and case.C % 64:
        out.add("fused-ragged-slice")
    return out


BRANCHES = {
    F32: {"flat", "flat-2vec", "flat-256vec", "flat-ld", "flat-ragged-trip", "generic", "generic-chunks", "generic-ragged-chunk", "generic-32chunks",
          "generic-ragged-trip", "apply-blocks", "apply-ragged-block", "reduce-cg8", "reduce-cg8-boundary", "reduce-cg16", "reduce-unrolled",
          "reduce-unrolled-tail", "reduce-no-unrolled", "reduce-blocks", "reduce-ragged-block", "fused-ragged-slice"},
    BF: {"flat", "flat-1vec", "flat-256vec", "flat-ld", "flat-ragged-trip", "generic", "generic-chunks", "generic-ragged-chunk", "generic-ragged-trip",
         "apply-blocks", "apply-ragged-block", "reduce-cg8", "reduce-cg8-boundary", "reduce-cg16", "reduce-unrolled", "reduce-unrolled-tail",
         "reduce-no-unrolled", "reduce-blocks", "reduce-ragged-block", "fused-ragged-slice"},
}


# ---- bars -------------------------------------------------------------------------------------------------------------------------
def red_bound(terms, dim=0):
    """2^-24 (sqrt(n) + 8) sum |t_i| per channel; terms: float64 [n, C] (summed over `dim`)"""
    return U * (math.sqrt(terms.shape[dim]) + 8.0) * terms.abs().sum(dim)


def red_ratio(got, ref, bound):
    """worst err / bound over the channels (a zero bound admits only the exact value; NaN stays NaN)"""
    err = (got.detach().to(F64) - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(err), torch.full_like(err, math.nan), r)
    return float(r.max()) if not bool(torch.isnan(r).any()) else math.nan


def elem_ratio(got, ref, cal, dtype):
    err, e = rel_err(got, ref), rel_err(cal, ref)
    bar = max(4.0 * e, 1e-6) if dtype == F32 else 3.0 * e
    return err / bar if bar > 0.0 else (0.0 if err == 0.0 else math.inf)


ELEMENTWISE = ("y", "y0", "dz", "g", "y_fused", "dz_fused", "y_chain", "dz_chain")


def ratios(got, ref, cal, bounds, dtype, names=None):
    """err / bar per output: element-wise outputs against the calibration model, everything else against its derived bound"""
    out = {}
    for name in (names if names is not None else got.keys()):
        if name.startswith("_"):
            continue
        if name in ELEMENTWISE:
            out[name] = elem_ratio(got[name], ref[name], cal[name], dtype)
        else:
            out[name] = red_ratio(got[name], ref[name], bounds[name])
    return out


def within(r):
    return all(v <= 1.0 for v in r.values())


# ---- formulas ---------------------------------------------------------------------------------------------------------------------
def _act(v, act, slope=SLOPE):
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    return v


def _act_grad(src, act, mutant=None):
    if act == ACT_NONE:
        return torch.ones_like(src)
    pos = (src >= 0) if mutant == "mask_ge" else (src > 0)
    lo = 0.0 if (act == ACT_RELU or mutant == "leaky0") else SLOPE
    return torch.where(pos, torch.ones_like(src), torch.full_like(src, lo))


def _neighbour(v, vw):
    """the last 16-byte channel vector takes the values of the one before it"""
    v = v.clone()
    v[-vw:] = v[-2 * vw:-vw]
    return v


def _keep(rows, mutant):
    """row indices a reduction visits"""
    if mutant == "drop_last_row":
        return torch.arange(rows - 1)
    if mutant == "drop_tail_row" and rows >= 2:
        return torch.cat((torch.arange(rows - 2), torch.tensor([rows - 1])))
    return torch.arange(rows)


def apply_fwd(z, scale, shift, res, act, vw, model=None, mutant=None):
    """y = act(z * scale + shift + res); scale / shift None: the coefficient-free pass"""
    dt, rnd = _arith(model)
    v = z.to(dt)
    if scale is not None:
        sc, sh = scale.to(dt), shift.to(dt)
        if mutant == "vec_neighbour":
            sc, sh = _neighbour(sc, vw), _neighbour(sh, vw)
        v = v * sc + sh
    if res is not None and mutant != "no_residual":
        v = v + res.to(dt)
    y = _act(v, act, 0.0 if mutant == "leaky0" else SLOPE)
    if mutant == "drop_last_row":
        y = y.clone()
        y[-1] = 0
    return rnd(y)


def bwd_g(dy, src, act, model=None, mutant=None):
    """g = dy * act'(src): src is y, or the pre-activation z * fscale + fshift"""
    dt, _ = _arith(model)
    return dy.to(dt) * _act_grad(src.to(dt), act, mutant)


def bwd_sums(g, z, mean, rstd, mutant=None):
    """float64 terms [n, C] of sum g and sum g zhat"""
    k = _keep(g.shape[0], mutant)
    g, z = g.to(F64)[k], z.to(F64)[k]
    return g, g * (z - mean.to(F64)) * rstd.to(F64)


def bwd_dz(g, z, mean, rstd, gamma, sum_g, sum_gz, M, vw, model=None, mutant=None):
    dt, rnd = _arith(model)
    mu, rs, gm, sg, sgz = (t.to(dt) for t in (mean, rstd, gamma, sum_g, sum_gz))
    if mutant == "vec_neighbour":
        mu, rs, gm, sg, sgz = (_neighbour(t, vw) for t in (mu, rs, gm, sg, sgz))
    zhat = (z.to(dt) - mu) * rs
    inner = g.to(dt) - zhat * (sgz / M)
    if mutant != "no_sum_g":
        inner = inner - sg / M
    dz = gm * rs * inner
    if mutant == "drop_last_row":
        dz = dz.clone()
        dz[-1] = 0
    return rnd(dz)


def finish(mean, var, b_mean, b_var, gamma, beta, M, rm0, rv0, mutant=None):
    """(values, bounds) of what the finalize kernels write from a channel's mean and biased variance (float64 [C]):
    rstd, scale, shift and the running update; b_mean / b_var are the bounds of the inputs."""
    gamma, beta = gamma.to(F64), beta.to(F64)
    rstd = (var + EPS) ** -0.5
    b_rstd = 0.5 * rstd ** 3 * b_var + 3 * U * rstd          # 3 roundings: var + eps, sqrt, 1 / x; |d rstd / d var| = rstd^3 / 2 (rstd is convex and decreasing)
    scale = gamma * rstd
    b_scale = gamma.abs() * b_rstd + U * scale.abs()
    shift = beta - mean * scale
    b_shift = scale.abs() * b_mean + mean.abs() * b_scale + U * ((mean * scale).abs() + shift.abs())
    val = {"mean": mean, "rstd": rstd, "scale": scale, "shift": shift}
    bnd = {"mean": b_mean, "rstd": b_rstd, "scale": b_scale, "shift": b_shift}
    if rm0 is not None:
        unb = (M / (M - 1.0)) if M > 1 else 1.0
        if mutant == "swap_unbias":                             # the update takes the biased variance
            unb = 1.0
        val["running_mean"] = (1 - MOM) * rm0.to(F64) + MOM * mean
        val["running_var"] = (1 - MOM) * rv0.to(F64) + MOM * var * unb
        bnd["running_mean"] = MOM * b_mean + 2 * U * ((1 - MOM) * rm0.to(F64).abs() + MOM * mean.abs())
        bnd["running_var"] = MOM * unb * b_var + 3 * U * ((1 - MOM) * rv0.to(F64).abs() + MOM * var * unb)
    return val, bnd


def stats_direct(z, sh, mutant=None):
    """float64 mean / biased variance of z [rows, C] with their bounds as the shifted-sums route (colstats -> bn_finalize) forms them:
    d = z - sh, mean = sum d / M + sh, var = sum d^2 / M - (sum d / M)^2.  The terms are those of the sums that route takes."""
    k = _keep(z.shape[0], mutant)
    M = z.shape[0]
    d = z.to(F64)[k] - (sh.to(F64) if sh is not None else 0.0)
    dm = d.sum(0) / M
    mean = dm + (sh.to(F64) if sh is not None else 0.0)
    var = ((d * d).sum(0) / M - dm * dm).clamp_min(0.0)
    b_dm = red_bound(d / M)
    b_mean = b_dm + (U * mean.abs() if sh is not None else 0.0)     # (the rounding of dm + shift)
    b_var = red_bound(d * d / M) + 2 * dm.abs() * b_dm              # d var / d dm = -2 dm
    return mean, var, b_mean, b_var


def stats_centred(z):
    """float64 mean / biased variance with the bounds of a route that sums centred squares (tile statistics + Chan combine)"""
    zz = z.to(F64)
    M = zz.shape[0]
    mean = zz.mean(0)
    c2 = (zz - mean) ** 2
    return mean, c2.sum(0) / M, red_bound(zz / M), red_bound(c2 / M)


def tile_table(z, rpt, about=None):
    """float64 per-tile (mean, M2) [tiles, C, 2] of z [rows, C] with the bounds of an f32 evaluation of each tile's sums.
    about: [tiles, C] - M2 is taken about these centres instead of the float64 tile means.  The GPU test passes the means the launch
    STORED (their float64 values): the launch sums squares about its own f32 mean m', and sum (v - m')^2 = M2 + n (m' - m)^2 is another
    number than M2 wherever M2 is small against n ulp(m)^2 - the pair (m', M2 about m') is what the Chan combine consumes.  The mean
    column is held to the float64 mean either way."""
    zz = z.to(F64)
    rows, C = zz.shape
    tiles = -(-rows // rpt)
    tab, bnd = torch.zeros((tiles, C, 2), dtype=F64), torch.zeros((tiles, C, 2), dtype=F64)
    for t in range(tiles):
        blk = zz[t * rpt:min(rows, (t + 1) * rpt)]
        m = blk.mean(0)
        c2 = (blk - (m if about is None else about[t].to(F64))) ** 2
        tab[t, :, 0], tab[t, :, 1] = m, c2.sum(0)
        bnd[t, :, 0], bnd[t, :, 1] = red_bound(blk / blk.shape[0]), red_bound(c2)
    return tab, bnd


def chan(table, rows, rpt, mutant=None):
    """Chan et al. combine of a tile table (float64 of the f32 table the launch reads): mean, biased variance, M2 and their bounds.
    The sums behind them: mean = sum n_t m_t / M (n = tiles terms), M2 = sum M2_t + sum n_t (m_t - mean)^2 (2 tiles terms)."""
    tab = table.to(F64)
    tiles = tab.shape[0]
    n = torch.full((tiles,), float(rpt), dtype=F64)
    if mutant != "ragged_full":
        n[-1] = rows - (tiles - 1) * rpt
    if mutant == "drop_last_tile":
        tab, n = tab[:-1], n[:-1]
    w = (n / rows)[:, None]
    mean = (n[:, None] * tab[..., 0]).sum(0) / n.sum()           # (exact for the constant channels: small dyadic values)
    between = n[:, None] * (tab[..., 0] - mean) ** 2
    m2 = tab[..., 1].sum(0) + between.sum(0)
    b_mean = red_bound(w * tab[..., 0])
    b_m2 = red_bound(torch.cat((tab[..., 1], between), 0))
    return mean, m2 / rows, m2, b_mean, b_m2 / rows, b_m2


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id C ld col0 rows family act residual from_z g_out acc track det seed")
FAMILIES = ("plain", "offset", "const")


def rnd_to(t, dtype):
    """what a kernel of `dtype` is given, back in f32"""
    return t.float() if dtype == F32 else _rb(t.float())


def make_z(family, rows, C, g):
    """plain: mean 0.3, std 0.8.  offset: mean 30, std 0.5 (the cancellation case).  const: plain with every fourth channel a constant
    0.25 .. 1.25 (small dyadic values: exact in bf16, and so are their sums, so var = 0 and rstd = eps^-1/2 in every arithmetic)."""
    z = torch.randn((rows, C), generator=g)
    if family == "offset":
        return z * 0.5 + 30.0
    z = z * 0.8 + 0.3
    if family == "const":
        z[:, ::4] = 0.25 * (1 + (torch.arange(C)[::4] % 5)).float()
    return z


def tie_mask(z, fscale, fshift):
    """elements whose float64 pre-activation z * fscale + fshift is within 2^-20 (|z fscale| + |fshift|) of zero: a contracted f32
    evaluation may put them on either side"""
    p = z.to(F64) * fscale.to(F64)
    return (p + fshift.to(F64)).abs() <= 2.0 ** -20 * (p.abs() + fshift.to(F64).abs())


def _coeffs(z, gamma, beta):
    zz = z.to(F64)
    mean, var = zz.mean(0), zz.var(0, unbiased=False)
    rstd = (var + EPS) ** -0.5
    return mean.float(), rstd.float(), (gamma.to(F64) * rstd).float(), (beta.to(F64) - mean * gamma.to(F64) * rstd).float()


def move_ties(z, gamma, beta, dtype):
    """z-derived masks: elements on a tie are moved away (+0.5 before rounding); (z, (mean, rstd, scale, shift)) of the moved tensor"""
    for _ in range(8):
        co = _coeffs(z, gamma, beta)
        t = tie_mask(z, co[2], co[3])
        if not bool(t.any()):
            return z, co
        z = rnd_to(torch.where(t, z + 0.5, z), dtype)
    raise AssertionError("ties remain")


def shape_inputs(case, dtype):
    g = torch.Generator().manual_seed(case.seed)
    rows, C = case.rows, case.C
    z = rnd_to(make_z(case.family, rows, C, g), dtype)
    dy = rnd_to(torch.randn((rows, C), generator=g), dtype)
    res = rnd_to(torch.randn((rows, C), generator=g), dtype) if case.residual else None
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm0, rv0 = (torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5) if case.track else (None, None)
    acc0 = torch.randn((2, C), generator=g) if case.acc else None
    z, (mean, rstd, scale, shift) = move_ties(z, gamma, beta, dtype) if case.from_z else (z, _coeffs(z, gamma, beta))
    sh = z[0].clone() if case.family != "plain" else None          # colstats' shift: the first row; none on the plain family
    return dict(z=z, dy=dy, res=res, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, acc0=acc0, mean=mean, rstd=rstd, scale=scale, shift=shift,
                stat_shift=sh)


def shape_eval(inp, case, dtype, model=None, mutant=None):
    """the outputs of every launch of one shape case.  Models evaluate the element-wise outputs only."""
    vw, M = ve(dtype), case.rows
    z, dy, res = inp["z"], inp["dy"], inp["res"]
    out = {}
    out["y"] = apply_fwd(z, inp["scale"], inp["shift"], res, case.act, vw, model, mutant)
    if case.ld is None:
        out["y0"] = apply_fwd(z, None, None, res, case.act, vw, model, mutant)
    # backward launches on host-made inputs: y from the float64 forward, rounded to the dtype; sums from float64
    src = inp["pre"] if case.from_z else inp["y"]
    g = bwd_g(dy, src, case.act, model, mutant)
    _, rnd = _arith(model)
    if case.g_out:
        out["g"] = rnd(dy.to(g.dtype) if mutant == "g_before_mask" else g)
    out["dz"] = bwd_dz(g, z, inp["mean"], inp["rstd"], inp["gamma"], inp["sum_g"], inp["sum_gz"], M, vw, model, mutant)
    if model is not None:
        return out
    bnd = {}
    # forward statistics: colstats (adds into non-zero buffers) -> bn_finalize
    sh = inp["stat_shift"]
    k = _keep(M, mutant)
    d = z.to(F64)[k] - (sh.to(F64) if sh is not None else 0.0)
    out["sum"], out["sumsq"] = SUM0 + d.sum(0), SUMSQ0 + (d * d).sum(0)
    bnd["sum"] = red_bound(torch.cat((d, torch.full((1, case.C), SUM0, dtype=F64))))
    bnd["sumsq"] = red_bound(torch.cat((d * d, torch.full((1, case.C), SUMSQ0, dtype=F64))))
    mean, var, b_mean, b_var = stats_direct(z, sh, mutant)
    v, b = finish(mean, var, b_mean, b_var, inp["gamma"], inp["beta"], M, inp["rm0"], inp["rv0"], mutant)
    out.update({"fin_" + n: t for n, t in v.items()})
    bnd.update({"fin_" + n: t for n, t in b.items()})
    # col_tile_stats -> bn_finalize_tiles (centred squares)
    zt = z[k] if mutant in ("drop_last_row", "drop_tail_row") else z
    tab, tb = tile_table(zt, TILE_ROWS)
    if zt.shape[0] == M:
        out["table"], bnd["table"] = tab, tb
    mean, var, b_mean, b_var = stats_centred(zt)
    v, b = finish(mean, var, b_mean, b_var, inp["gamma"], inp["beta"], M, inp["rm0"], inp["rv0"], mutant)
    out.update({"til_" + n: t for n, t in v.items()})
    bnd.update({"til_" + n: t for n, t in b.items()})
    # bn_act_bwd_reduce (adds into non-zero buffers)
    tg, tgz = bwd_sums(g, z, inp["mean"], inp["rstd"], mutant)
    out["sum_g"], out["sum_gz"] = SUM0 + tg.sum(0), SUMSQ0 + tgz.sum(0)
    bnd["sum_g"] = red_bound(torch.cat((tg, torch.full((1, case.C), SUM0, dtype=F64))))
    bnd["sum_gz"] = red_bound(torch.cat((tgz, torch.full((1, case.C), SUMSQ0, dtype=F64))))
    if case.acc:
        a0 = inp["acc0"].to(F64)
        out["dbeta"], out["dgamma"] = a0[0] + inp["sum_g"].to(F64), a0[1] + inp["sum_gz"].to(F64)
        bnd["dbeta"] = red_bound(torch.stack((a0[0], inp["sum_g"].to(F64))))
        bnd["dgamma"] = red_bound(torch.stack((a0[1], inp["sum_gz"].to(F64))))
    out["_bounds"] = bnd
    return out


@lru_cache(maxsize=4)
def shape_setup(case, dtype):
    """(inputs as the kernels of `dtype` see them, float64 reference, calibration model, bounds)"""
    inp = shape_inputs(case, dtype)
    z = inp["z"].to(F64)
    pre = z * inp["scale"].to(F64) + inp["shift"].to(F64)
    inp["pre"] = pre
    y64 = apply_fwd(inp["z"], inp["scale"], inp["shift"], inp["res"], case.act, ve(dtype))
    inp["y"] = rnd_to(y64, dtype)
    g = bwd_g(inp["dy"], pre if case.from_z else inp["y"], case.act)
    tg, tgz = bwd_sums(g, inp["z"], inp["mean"], inp["rstd"])
    inp["sum_g"], inp["sum_gz"] = tg.sum(0).float(), tgz.sum(0).float()
    ref = shape_eval(inp, case, dtype)
    bounds = ref.pop("_bounds")
    cal = shape_eval(inp, case, dtype, model="f32" if dtype == F32 else "bf16")
    return inp, ref, cal, bounds


W_NARROW = ((8, None), (32, None), (48, 304), (64, None), (72, None), (136, None))
W_WIDE = ((256, 512), (1024, None), (2048, None))
ROWS_NARROW = (1, 5, 63, 64, 65, 127, 129, 191, 257)
ROWS_LONG = (1000, 6277)
ROWS_WIDE = (5, 130)


def _mk(i, C, ld, rows):
    fam = FAMILIES[i % 3]
    act = (ACT_NONE, ACT_RELU, ACT_LEAKY)[(i // 3 + i) % 3]
    residual = i % 2 == 0
    from_z = (not residual) and act != ACT_NONE and (i // 2) % 2 == 0
    cid = f"c{C}{'in' + str(ld) if ld else ''}-r{rows}-{fam}-a{act}-{'res' if residual else 'fromz' if from_z else 'y'}"
    return Case(cid, C, ld, 8 if ld else 0, rows, fam, act, residual, from_z, (i // 2) % 2 == 1, (i // 3) % 2 == 0, i % 4 != 3,
                (C, rows) in ((136, 257), (64, 6277)), 7000 + i)


def shape_cases(dtype=None):
    out, i = [], 0
    for C, ld in W_NARROW:
        for rows in ROWS_NARROW:
            out.append(_mk(i, C, ld, rows))
            i += 1
        i += 1      # (shift the cycles from one width to the next)
    for C in (8, 64):
        for rows in ROWS_LONG:
            out.append(_mk(i, C, None, rows))
            i += 1
    for C, ld in W_WIDE:
        for rows in ROWS_WIDE:
            out.append(_mk(i, C, ld, rows))
            i += 1
    if dtype is not None:
        out = [c for c in out if not (c.C == 1024 and dtype != F32)]     # 1024: f32 only (in bf16 it is one more 128-vector flat case)
    return out


def shape_mutants(case, dtype):
    """The mutants that move at least one output of this case past its bar.  Rules:
    drop_last_row: the last row's outputs are not written and no sum sees it - visible wherever there is a last row.
    drop_tail_row: row M - 2 missing from the sums; needs M >= 2.
    vec_neighbour: needs two channel vectors.
    leaky0 / mask_ge / g_before_mask: need the activation; mask_ge needs exact zeros in y, which ReLU outputs are full of (the
      z-derived mask has no ties by construction); g_before_mask needs g_out.
    no_sum_g: the mean term of dz, sum g / M ~ M^-1/2 of an element of g: bf16 (3 x 2^-9 of max |dz| ~ 4 g) resolves it for certain up
      to M = 257 (0.06 against 0.024); the f32 runs carry it at M = 1000 and 6277.
    swap_unbias: the running update; var / M against the bound of running_var (M <= 6277: a relative 1.6e-4 against
      (sqrt(M) + 8) 2^-24 <= 5.3e-6), in every case with M > 1 that tracks - constant channels have neighbours that are not.
    no_residual: needs the residual."""
    out = ["drop_last_row"]
    if dtype == F32 or case.rows <= 257:
        out.append("no_sum_g")
    if case.rows >= 2:
        out.append("drop_tail_row")
    if case.C >= 2 * ve(dtype):
        out.append("vec_neighbour")
    if case.act == ACT_LEAKY:
        out.append("leaky0")
    if case.act == ACT_RELU and not case.from_z:
        out.append("mask_ge")
    if case.act != ACT_NONE and case.g_out:
        out.append("g_before_mask")
    if case.track and case.rows > 1:
        out.append("swap_unbias")
    if case.residual:
        out.append("no_residual")
    return out


ALL_SHAPE_MUTANTS = {"drop_last_row", "drop_tail_row", "vec_neighbour", "leaky0", "mask_ge", "g_before_mask", "no_sum_g", "swap_unbias",
                     "no_residual"}


# ---- tile tables: the one-wave and the wide finalize, the moments of a rank and the second stage, the fused launches ---------------
TCase = namedtuple("TCase", "id C tiles rpt rows family act residual track world seed")
TILES_WAVE = (1, 2, 63, 64, 65, "limit", "limit+1")
TILES_WIDE = (1023, 1024, 1025, 2051)


def tile_cases():
    out, i = [], 0
    for tiles in TILES_WAVE + TILES_WIDE:
        for C in (8, 72):
            n = BN_FUSED_TILES if tiles == "limit" else BN_FUSED_TILES + 1 if tiles == "limit+1" else tiles
            wide = tiles in TILES_WIDE
            fam = ("plain", "offset", "const")[i % 3]
            out.append(TCase(f"t{tiles}-c{C}-{fam}", C, n, 8, n * 8 - 3, fam, (ACT_RELU, ACT_LEAKY, ACT_NONE)[i % 3], (i // 2) % 2 == 0,
                             i % 3 != 1, (1, 2, 8)[i % 3], 8000 + i))
            i += 1
    return out


def tile_inputs(case, dtype):
    g = torch.Generator().manual_seed(case.seed)
    rows, C = case.rows, case.C
    z = rnd_to(make_z(case.family, rows, C, g), dtype)
    dy = rnd_to(torch.randn((rows, C), generator=g), dtype)
    res = rnd_to(torch.randn((rows, C), generator=g), dtype) if case.residual else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rm0, rv0 = (torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5) if case.track else (None, None)
    table = tile_table(z, case.rpt)[0].float()                     # host-made float64 table cast to f32
    mean, rstd, _, _ = _coeffs(z, gamma, beta)
    pad = case.tiles * case.rpt - rows
    tg, tgz = bwd_sums(dy, z, mean, rstd)
    part = torch.stack([torch.cat((t, t.new_zeros((pad, C)))).view(case.tiles, case.rpt, C).sum(1) for t in (tg, tgz)], -1).float()
    # the other ranks of the second stage: moments of tensors of the same family, host-made
    others = [stats_centred(rnd_to(make_z(case.family, rows, C, g), dtype)) for _ in range(case.world - 1)]
    return dict(z=z, dy=dy, res=res, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, table=table, part=part, mean=mean, rstd=rstd,
                others=[torch.stack((m, v * rows), -1).float() for m, v, _, _ in others])


def tile_eval(inp, case, dtype, model=None, mutant=None):
    vw, M = ve(dtype), case.rows
    dt, rnd = _arith(model)
    out, bnd = {}, {}
    if model is None:
        mean, var, m2, b_mean, b_var, b_m2 = chan(inp["table"], M, case.rpt, mutant)
    else:   # the same combine in the model's arithmetic (one f32 pass over the tiles)
        tab = inp["table"].to(dt)
        n = torch.full((case.tiles, 1), float(case.rpt), dtype=dt)
        n[-1] = M - (case.tiles - 1) * case.rpt
        mean = (n * tab[..., 0]).sum(0) / M
        var = (tab[..., 1].sum(0) + (n * (tab[..., 0] - mean) ** 2).sum(0)) / M
    gamma, beta = inp["gamma"].to(dt), inp["beta"].to(dt)
    rstd = (var + EPS) ** -0.5
    # (above the limit the wrapper runs the two launches: same outputs)
    out["y_fused"] = apply_fwd(inp["z"], gamma * rstd, beta - mean * gamma * rstd, inp["res"], case.act, vw, model, mutant)
    part = inp["part"].to(dt)
    sg, sgz = part[..., 0].sum(0), part[..., 1].sum(0)
    out["dz_fused"] = bwd_dz(inp["dy"], inp["z"], inp["mean"], inp["rstd"], inp["gamma"], sg, sgz, M, vw, model, mutant)
    if model is not None:
        return out
    v, b = finish(mean, var, b_mean, b_var, inp["gamma"], inp["beta"], M, inp["rm0"], inp["rv0"], mutant)
    out.update(v)
    bnd.update(b)
    out["moments"] = torch.stack((mean, m2), -1)
    bnd["moments"] = torch.stack((b_mean, b_m2), -1)
    p64 = inp["part"].to(F64)
    out["sum_g"], out["sum_gz"] = SUM0 + p64[..., 0].sum(0), SUMSQ0 + p64[..., 1].sum(0)
    bnd["sum_g"] = red_bound(torch.cat((p64[..., 0], torch.full((1, case.C), SUM0, dtype=F64))))
    bnd["sum_gz"] = red_bound(torch.cat((p64[..., 1], torch.full((1, case.C), SUMSQ0, dtype=F64))))
    out["fsum_g"], out["fsum_gz"] = p64[..., 0].sum(0), p64[..., 1].sum(0)      # the fused launch: zero on entry
    bnd["fsum_g"], bnd["fsum_gz"] = red_bound(p64[..., 0]), red_bound(p64[..., 1])
    # second stage: this rank's moments (host-made from float64) gathered with the other ranks', world tiles of `rows` rows each
    own = torch.stack((mean, m2), -1).float() if mutant is None else torch.stack(chan(inp["table"], M, case.rpt)[0:3:2], -1).float()
    gathered = torch.stack([own] + inp["others"])
    out["_gathered"] = gathered
    mean2, var2, _, b_mean2, b_var2, _ = chan(gathered, M * case.world, M, mutant if mutant == "drop_last_tile" and case.world > 1 else None)
    v, b = finish(mean2, var2, b_mean2, b_var2, inp["gamma"], inp["beta"], M * case.world, inp["rm0"],
                  inp["rv0"], mutant)
    out.update({"st2_" + n: t for n, t in v.items()})
    bnd.update({"st2_" + n: t for n, t in b.items()})
    out["_bounds"] = bnd
    return out


@lru_cache(maxsize=4)
def tile_setup(case, dtype):
    inp = tile_inputs(case, dtype)
    ref = tile_eval(inp, case, dtype)
    bounds = ref.pop("_bounds")
    inp["gathered"] = ref.pop("_gathered")
    cal = tile_eval(inp, case, dtype, model="f32" if dtype == F32 else "bf16")
    return inp, ref, cal, bounds


def tile_mutants(case):
    """ragged_full: the last tile's 5 rows counted as 8 - needs a second tile to weigh against.  drop_last_tile: the wide combine's
    tail.  swap_unbias: as in shape_mutants."""
    out = []
    if case.tiles >= 2:
        out.append("ragged_full")
    if wide_finalize(case.tiles):
        out.append("drop_last_tile")
    if case.track:
        out.append("swap_unbias")
    return out


# ---- chains: z -> statistics -> apply, dy -> reduce -> apply against float64 BatchNorm forward and backward -----------------------
def bn_forward(z, gamma, beta, res, act):
    """float64, autograd-friendly: act(gamma (z - mu) rstd + beta + res) with the batch statistics of z [rows, C]"""
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    y = gamma * (z - mu) * (var + EPS) ** -0.5 + beta
    if res is not None:
        y = y + res
    return _act(y, act)


def chain_eval(z, dy, res, gamma, beta, act, vw, model=None):
    """{y_chain, dz_chain, dbeta, dgamma} by the explicit formulas (test_bn_ref_host.py holds them to autograd of F.batch_norm)"""
    dt, rnd = _arith(model)
    zz, gm, bt = z.to(dt), gamma.to(dt), beta.to(dt)
    M = zz.shape[0]
    mu = zz.mean(0)
    var = ((zz - mu) ** 2).mean(0)
    rstd = (var + EPS) ** -0.5
    y = rnd(apply_fwd(zz, gm * rstd, bt - mu * gm * rstd, res, act, vw, model))
    g = bwd_g(dy, y, act, model)
    zhat = (zz - mu) * rstd
    sg, sgz = g.sum(0), (g * zhat).sum(0)
    return {"y_chain": y, "dz_chain": bwd_dz(g, zz, mu, rstd, gm, sg, sgz, M, vw, model), "dbeta": sg, "dgamma": sgz}


def chain_setup(C, rows, dtype, seed):
    """plain family, ReLU, no residual (the mask comes from the launch's own y, so pre-activation ties are moved away as for the
    z-derived masks).  Bounds of dbeta / dgamma: their own sums plus the statistics' bounds through d zhat = rstd d mean + (z - mu) d rstd."""
    g = torch.Generator().manual_seed(seed)
    z = rnd_to(make_z("plain", rows, C, g), dtype)
    dy = rnd_to(torch.randn((rows, C), generator=g), dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    z, _ = move_ties(z, gamma, beta, dtype)
    ref = chain_eval(z, dy, None, gamma, beta, ACT_RELU, ve(dtype))
    cal = chain_eval(z, dy, None, gamma, beta, ACT_RELU, ve(dtype), model="f32" if dtype == F32 else "bf16")
    mean, var, b_mean, b_var = stats_direct(z, None)
    _, b = finish(mean, var, b_mean, b_var, gamma, beta, rows, None, None)
    gg = bwd_g(dy, ref["y_chain"], ACT_RELU)
    tg, tgz = bwd_sums(gg, z, mean, (var + EPS) ** -0.5)
    prop = (gg.abs() * ((var + EPS) ** -0.5 * b["mean"] + (z.to(F64) - mean).abs() * b["rstd"])).sum(0)
    return dict(z=z, dy=dy, gamma=gamma, beta=beta), ref, cal, {"dbeta": red_bound(tg), "dgamma": red_bound(tgz) + prop}


CHAIN_WIDTHS = ((64, None, "flat"), (72, None, "generic"), (256, 512, "flat-ld"))
