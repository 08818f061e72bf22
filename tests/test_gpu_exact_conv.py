"""Bit-exact forward parity on integer-lattice inputs (tests/_lattice.py): ops.conv2d on every implicit-GEMM tile, split-K, the fused
epilogue, channel slices, periodic residuals, ops.linear, the small-Cin stems and the depth-wise conv, against float64 on the CPU.

f32 outputs must be torch.equal to the reference, bf16 outputs to ref.to(bfloat16): there is no tolerance.  The shape tables are the
ones of test_gpu_ops / test_gpu_igemm_big / test_gpu_igemm_persistent; test_lattice_host.py imports the tables of THIS file and checks
every case's preconditions (2^24, bf16 magnitude) on the CPU.

Entry points held bit-exact here: cavp_conv2d_nhwc_aux (tiles 0..14, split-K 1/2/3/7, scale / shift / per-image bias / residual /
ReLU / leaky ReLU, ld != C views, res_rows), cavp_pack_weight_ohwi, cavp_conv3x3_smallcin_nchw, cavp_conv_smallcin_kxk_nchw,
cavp_dwconv3x3_nhwc_aux (no activation), cavp_pack_dwconv_weight.  GELU and aux_mode are not exact on integers and stay with their
tolerance tests."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _lattice as L
from tests.test_gpu_igemm_big import CASES as BIG_CASES
from tests.test_gpu_igemm_persistent import COUT as PERSIST_COUT, FWD as PERSIST_FWD, MIN_WG, _wg
from tests.test_gpu_ops import CONV_CASES, DEV, _to_nhwc_dev

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
DTYPES = [F32, BF]
DT_ID = {F32: "f32", BF: "bf16"}
TILES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14]   # both dtypes; tile 10 (256 x 256) is bf16 only, Cout % 8 == 0
BIG_TILE = 10

# two launches with more logical workgroups than twice the persistent grid (every workgroup walks >= 2 tiles)
PERSIST_CASES = [("persist_" + nm,) + PERSIST_FWD[nm][:3] + (PERSIST_FWD[nm][4], PERSIST_COUT) + PERSIST_FWD[nm][5:9]
                 for nm in ("1x1_k1", "3x3_ragged")]
PERSIST_TILES = [1, 8, 9, 12]

FWD_TABLE = {c[0]: c for c in CONV_CASES}
FWD_TABLE.update({"big_" + c[0]: c for c in BIG_CASES})
FWD_TABLE.update({c[0]: c for c in PERSIST_CASES})


def _ops():
    from cavp_amd import ops
    return ops


def _seed(name, salt=0):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003 + 1000 * salt


@functools.lru_cache(maxsize=2)
def fwd_problem(key):
    """lattice inputs + float64 reference (NHWC) of one FWD_TABLE case, computed once and shared by tile / split / dtype"""
    name, n, h, w, cin, cout, k, s, p, d = FWD_TABLE[key]
    K = cin * k * k
    x = L.activations((n, cin, h, w), K, _seed(key, 1))
    wt = L.weights((cout, cin, k, k), _seed(key, 2))
    ref = L.ref64_conv(x, wt, s, p, d).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=wt, conv=(k, s, p, d), ref=ref, want={dt: L.expected(ref, dt) for dt in DTYPES})


def _launch_plain(key, dtype, **kw):
    ops = _ops()
    pb = fwd_problem(key)
    k, s, p, d = pb["conv"]
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], key)
    xv, _ = _to_nhwc_dev(pb["x"], dtype)
    out = torch.full(tuple(pb["ref"].shape), float("nan"), dtype=dtype, device=DEV)
    ops.conv2d(xv, ops.pack_weight(pb["w"].to(DEV), dtype), out, kh=k, kw=k, stride=s, pad=p, dil=d, **kw)
    return out, pb


def _tile_params(names, tiles, with_big):
    out = []
    for nm in names:
        for dt in DTYPES:
            ts = list(tiles) + ([BIG_TILE] if with_big and dt == BF and FWD_TABLE[nm][5] % 8 == 0 else [])
            out += [pytest.param(nm, dt, t, id=f"{nm}-{DT_ID[dt]}-tile{t}") for t in ts]
    return out


@pytest.mark.parametrize("key,dtype,tile", _tile_params([c[0] for c in CONV_CASES], TILES, True))
def test_conv_tiles_exact(key, dtype, tile):
    """every tile id on every layer shape of test_gpu_ops: K tails (Cin 304, 48), dead taps, stride 2 on odd extents, ragged images"""
    out, pb = _launch_plain(key, dtype, tile=tile)
    L.assert_exact(out, pb["want"][dtype], dtype, f"{key}/tile{tile}", "nhwc")


@pytest.mark.parametrize("key,dtype,tile", _tile_params(["big_" + c[0] for c in BIG_CASES], [0, 1], True))
def test_conv_big_tile_shapes_exact(key, dtype, tile):
    """the 256 x 256 tile's own table (launches that cross output tiles, one-K-tile streams, channel tails), the planner's choice and
    the 128 x 128 tile on the same inputs"""
    out, pb = _launch_plain(key, dtype, tile=tile)
    L.assert_exact(out, pb["want"][dtype], dtype, f"{key}/tile{tile}", "nhwc")


@pytest.mark.parametrize("key,dtype,tile", _tile_params([c[0] for c in PERSIST_CASES], PERSIST_TILES, False))
def test_conv_persistent_launches_exact(key, dtype, tile):
    name, n, h, w, cin, cout, k, s, p, d = FWD_TABLE[key]
    rows = fwd_problem(key)["ref"].numel() // cout
    assert _wg(tile, rows, cout) >= MIN_WG, "the case no longer exceeds twice the persistent grid"
    out, pb = _launch_plain(key, dtype, tile=tile)
    L.assert_exact(out, pb["want"][dtype], dtype, f"{key}/tile{tile}", "nhwc")


# ---- split-K ----------------------------------------------------------------------------------------------------------------
SPLITK_SHAPES = {"256_96": (1, 14, 14, 256, 96), "304_ktail_48": (2, 9, 11, 304, 48)}


@functools.lru_cache(maxsize=2)
def splitk_problem(shape):
    n, h, w, cin, cout = SPLITK_SHAPES[shape]
    x = L.activations((n, cin, h, w), cin * 9, _seed(shape, 3))
    wt = L.weights((cout, cin, 3, 3), _seed(shape, 4))
    bias = L.ints((cout,), -8, 8, _seed(shape, 5))
    ref = L.ref64_conv(x, wt, 1, 1, 1, shift=bias, act=L.ACT_RELU).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=wt, bias=bias, ref=ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("splitk", [1, 2, 3, 7])
@pytest.mark.parametrize("shape", list(SPLITK_SHAPES))
def test_conv_splitk_exact(shape, splitk, dtype):
    ops = _ops()
    pb = splitk_problem(shape)
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], shape)
    xv, _ = _to_nhwc_dev(pb["x"], dtype)
    out = torch.full(tuple(pb["ref"].shape), float("nan"), dtype=dtype, device=DEV)
    ops.conv2d(xv, ops.pack_weight(pb["w"].to(DEV), dtype), out, kh=3, kw=3, pad=1, shift=pb["bias"].to(DEV), act=ops.ACT_RELU,
               splitk=splitk)
    L.assert_exact(out, pb["ref"], dtype, f"{shape}/splitk{splitk}", "nhwc")


# ---- small Cout (scalar-tail epilogue) ----------------------------------------------------------------------------------------
SMALL_COUT = [2, 22, 71, 24]


@functools.lru_cache(maxsize=4)
def small_cout_problem(cout):
    x = L.activations((2, 256, 12, 10), 256, 60 + cout)
    wt = L.weights((cout, 256, 1, 1), 70 + cout)
    b = L.ints((cout,), -8, 8, 80 + cout)
    return dict(x=x, w=wt, b=b, ref=L.ref64_conv(x, wt, shift=b).permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cout", SMALL_COUT)
def test_conv_small_cout_exact(cout, dtype):
    ops = _ops()
    pb = small_cout_problem(cout)
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], f"cls{cout}")
    xv, _ = _to_nhwc_dev(pb["x"], dtype)
    out = torch.full((2, 12, 10, cout), float("nan"), dtype=dtype, device=DEV)
    ops.conv2d(xv, ops.pack_weight(pb["w"].to(DEV), dtype), out, shift=pb["b"].to(DEV))
    L.assert_exact(out, pb["ref"], dtype, f"cls{cout}", "nhwc")


# ---- the full epilogue on channel slices -----------------------------------------------------------------------------------------
EPI_SHAPE = (3, 19, 21, 64, 48)
EPI_ACTS = [L.ACT_NONE, L.ACT_RELU, L.ACT_LEAKY]


@functools.lru_cache(maxsize=3)
def epilogue_problem(act):
    """gain 4: the sums stay below 64 so that scale 4 keeps the result inside the bf16 integer range, scale 1/4 gives quarter steps"""
    n, h, w, cin, cout = EPI_SHAPE
    x = L.activations((n, cin, h, w), cin, 9, gain=4.0)
    wt = L.weights((cout, cin, 1, 1), 10)
    sc, sh = L.pow2_scales(cout, 11), L.ints((cout,), -8, 8, 12)
    nb, res = L.ints((n, cout), -4, 4, 13), L.ints((n, cout, h, w), -4, 4, 14)
    ref = L.ref64_conv(x, wt, scale=sc, shift=sh, nbias=nb, residual=res, act=act).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=wt, sc=sc, sh=sh, nb=nb, res=res, ref=ref)


@pytest.mark.parametrize("dtype,tile", [(F32, 0), (F32, 1), (F32, 6), (BF, 0), (BF, 1), (BF, 6), (BF, BIG_TILE)],
                         ids=["f32-auto", "f32-tile1", "f32-tile6", "bf16-auto", "bf16-tile1", "bf16-tile6", "bf16-tile10"])
@pytest.mark.parametrize("act", EPI_ACTS)
def test_conv_epilogue_exact(act, dtype, tile):
    """act((conv + nbias) * 2^k + shift + residual) reading a channel slice of x and of the residual and writing the [256, 304) slice of
    a wide buffer, whose other channels must stay untouched.  (bf16 + leaky: the f32 product 0.01 * y is then rounded once.)"""
    ops = _ops()
    n, h, w, cin, cout = EPI_SHAPE
    pb = epilogue_problem(act)
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], f"epilogue act{act}")
    xv, _ = _to_nhwc_dev(pb["x"], dtype, ld=96, c0=16)
    rv, _ = _to_nhwc_dev(pb["res"], dtype, ld=64, c0=8)
    big = torch.full((n, h, w, 304), -3.0, dtype=dtype, device=DEV)
    out = big[..., 256:304]
    ops.conv2d(xv, ops.pack_weight(pb["w"].to(DEV), dtype), out, scale=pb["sc"].to(DEV), shift=pb["sh"].to(DEV),
               nbias=pb["nb"].to(DEV), residual=rv, act=act, tile=tile)
    L.assert_exact(out, pb["ref"], dtype, f"epilogue act{act} tile{tile}", "nhwc")
    assert float((big[..., :256].float() + 3.0).abs().max()) == 0.0, "wrote outside its channel slice"


# ---- batch-periodic residual -------------------------------------------------------------------------------------------------------
RES_ROWS_SHAPE = (4, 512, 96, 256)   # 2048 token rows, residual period 1024 rows


@functools.lru_cache(maxsize=1)
def res_rows_problem():
    n, t, cin, cout = RES_ROWS_SHAPE
    x = L.activations((n, cin, 1, t), cin, 31)
    wt = L.weights((cout, cin, 1, 1), 32)
    bias = L.ints((cout,), -8, 8, 33)
    res = L.ints((n // 2, cout, 1, t), -4, 4, 35)
    ref = L.ref64_conv(x, wt, shift=bias, residual=torch.cat((res, res), 0)).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=wt, bias=bias, res=res, ref=ref)


@pytest.mark.parametrize("dtype,tile", [(F32, 0), (F32, 1), (BF, 0), (BF, 1), (BF, BIG_TILE)],
                         ids=["f32-auto", "f32-tile1", "bf16-auto", "bf16-tile1", "bf16-tile10"])
def test_conv_periodic_residual_exact(dtype, tile):
    ops = _ops()
    n, t, cin, cout = RES_ROWS_SHAPE
    pb = res_rows_problem()
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], "res_rows")
    xv, _ = _to_nhwc_dev(pb["x"], dtype)
    rv, _ = _to_nhwc_dev(pb["res"], dtype)
    out = torch.full((n, 1, t, cout), float("nan"), dtype=dtype, device=DEV)
    ops.conv2d(xv, ops.pack_weight(pb["w"].to(DEV), dtype), out, shift=pb["bias"].to(DEV), residual=rv, res_rows=(n // 2) * t,
               tile=tile)
    L.assert_exact(out, pb["ref"], dtype, f"periodic residual tile{tile}", "nhwc")


# ---- linear ---------------------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(2, 12288, 4096), (64, 4096, 304), (3, 2048, 256), (6272, 304, 1216)]


@functools.lru_cache(maxsize=1)
def linear_problem(shape):
    rows, cin, cout = shape
    x = L.activations((rows, cin), cin, 15)
    wt = L.weights((cout, cin), 16)
    b = L.ints((cout,), -8, 8, 17)
    return dict(x=x, w=wt, b=b, ref=L.ref64_linear(x, wt, b, L.ACT_RELU))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=["x".join(map(str, s)) for s in LINEAR_SHAPES])
def test_linear_exact(shape, dtype):
    ops = _ops()
    rows, cin, cout = shape
    pb = linear_problem(shape)
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], f"linear {shape}")
    out = torch.full((rows, cout), float("nan"), dtype=dtype, device=DEV)
    ops.linear(pb["x"].to(dtype).to(DEV), ops.pack_weight(pb["w"].to(DEV), dtype), out, bias=pb["b"].to(DEV), act=ops.ACT_RELU)
    L.assert_exact(out, pb["ref"], dtype, f"linear {rows}x{cin}->{cout}", ("row", "c"))


# ---- bf16 rounding probes: results in 256..2048 on purpose -------------------------------------------------------------------
PROBE_SHAPE = (1, 20, 20, 256, 256, 3)   # K = 2304
PROBE_PLANS = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (8, 0), (9, 0), (BIG_TILE, 0), (11, 0), (0, 2), (0, 3), (0, 7)]


@functools.lru_cache(maxsize=1)
def probe_problem():
    n, h, w, cin, cout, k = PROBE_SHAPE
    x, wt = L.biased_conv_inputs(n, cin, h, w, cout, k, 77)
    conv = L.ref64_conv(x, wt, 1, 1, 1)                        # NCHW, integers
    res = -L.expected(conv, BF).double()                       # bf16-representable: the rounded result, negated
    small = L.ints(tuple(conv.shape), -5, 5, 78).double()      # an ordinary small residual (the host mutation table uses it)
    return dict(x=x, w=wt, conv=conv, res=res, small=small)


def probe_preconditions(pb):
    """on the reference alone: most sums are in the range where bf16 drops integers, and the cancelled result is not zero"""
    a = pb["conv"].abs()
    assert float(((a >= 256) & (a <= 2048)).double().mean()) >= 0.6
    left = pb["conv"] + pb["res"]
    assert float(left.abs().max()) <= 8 and float((left != 0).double().mean()) >= 0.25


@pytest.mark.parametrize("tile,splitk", PROBE_PLANS, ids=[f"tile{t}-sk{s}" for t, s in PROBE_PLANS])
def test_bf16_rounds_once_after_the_residual(tile, splitk):
    """Early-rounding probe: residual = -bf16(conv).  The exact output is the small integer conv - bf16(conv); a kernel that rounds
    its accumulator (or a split-K partial) to bf16 before the residual is added returns zeros (or multiples of the bf16 step)."""
    ops = _ops()
    n, h, w, cin, cout, k = PROBE_SHAPE
    pb = probe_problem()
    probe_preconditions(pb)
    xv, _ = _to_nhwc_dev(pb["x"], BF)
    rv, _ = _to_nhwc_dev(pb["res"].float(), BF)
    wp = ops.pack_weight(pb["w"].to(DEV), BF)
    out = torch.full((n, h, w, cout), float("nan"), dtype=BF, device=DEV)
    ops.conv2d(xv, wp, out, kh=k, kw=k, pad=1, residual=rv, tile=tile, splitk=splitk)
    L.assert_exact(out, (pb["conv"] + pb["res"]).permute(0, 2, 3, 1), BF, f"cancelling residual tile{tile} sk{splitk}", "nhwc")
    rv2, _ = _to_nhwc_dev(pb["small"].float(), BF)
    out.fill_(float("nan"))
    ops.conv2d(xv, wp, out, kh=k, kw=k, pad=1, residual=rv2, tile=tile, splitk=splitk)
    L.assert_exact(out, (pb["conv"] + pb["small"]).permute(0, 2, 3, 1), BF, f"small residual tile{tile} sk{splitk}", "nhwc")


@pytest.mark.parametrize("tile,splitk", PROBE_PLANS, ids=[f"tile{t}-sk{s}" for t, s in PROBE_PLANS])
def test_bf16_ties_round_to_even(tile, splitk):
    """Tie probe: the same large sums without a residual must equal ref.to(bfloat16) - every odd integer in 256..512 and every
    n % 4 == 2 in 512..1024 is a tie, so truncation or round-half-up shows on thousands of elements."""
    ops = _ops()
    n, h, w, cin, cout, k = PROBE_SHAPE
    pb = probe_problem()
    ref = pb["conv"].permute(0, 2, 3, 1)
    assert int((L.expected(ref, BF) != L.truncate_to_bf16(ref)).sum()) >= 1000, "the probe must contain ties that round up"
    xv, _ = _to_nhwc_dev(pb["x"], BF)
    out = torch.full((n, h, w, cout), float("nan"), dtype=BF, device=DEV)
    ops.conv2d(xv, ops.pack_weight(pb["w"].to(DEV), BF), out, kh=k, kw=k, pad=1, tile=tile, splitk=splitk)
    L.assert_exact(out, ref, BF, f"ties tile{tile} sk{splitk}", "nhwc")


# ---- stems and PVT pieces -----------------------------------------------------------------------------------------------------------
STEM3_CASES = [(3, 2, (32, 40)), (1, 1, (96, 64)), (3, 2, (31, 45)), (3, 1, (6, 300)), (2, 2, (9, 515)), (3, 2, (224, 224))]


@functools.lru_cache(maxsize=2)
def stem3_problem(case):
    cin, stride, hw = case
    x = L.activations((2, cin, *hw), cin * 9, 18, gain=4.0)
    wt = L.weights((64, cin, 3, 3), 19)
    sc, sh = L.pow2_scales(64, 20), L.ints((64,), -8, 8, 21)
    ref = L.ref64_conv(x, wt, stride, 1, 1, scale=sc, shift=sh, act=L.ACT_RELU).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=wt, sc=sc, sh=sh, ref=ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", STEM3_CASES, ids=[f"cin{c}-s{s}-{h}x{w}" for c, s, (h, w) in STEM3_CASES])
def test_conv3x3_smallcin_exact(case, dtype):
    """(bf16 = the matrix-core stem: the f32 image and weights are split into bf16 hi + lo pairs; integers have no lo part)"""
    ops = _ops()
    cin, stride, hw = case
    pb = stem3_problem(case)
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], f"smallcin {case}")
    out = torch.full(tuple(pb["ref"].shape), float("nan"), dtype=dtype, device=DEV)
    ops.conv3x3_smallcin_nchw(pb["x"].to(DEV), pb["w"].to(DEV), out, stride=stride, scale=pb["sc"].to(DEV), shift=pb["sh"].to(DEV),
                              act=ops.ACT_RELU)
    L.assert_exact(out, pb["ref"], dtype, f"smallcin {case}", "nhwc")


PATCH_SHAPE = (2, 3, 64, 96, 64, 7, 4, 3)   # N, Cin, H, W, Cout, k, stride, pad


@functools.lru_cache(maxsize=1)
def patch_embed_problem():
    n, cin, h, w, cout, k, s, p = PATCH_SHAPE
    x = L.activations((n, cin, h, w), cin * k * k, 55)
    wt, b = L.weights((cout, cin, k, k), 56), L.ints((cout,), -8, 8, 57)
    return dict(x=x, w=wt, b=b, ref=L.ref64_conv(x, wt, s, p, 1, shift=b).permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_conv_smallcin_kxk_exact(dtype):
    ops = _ops()
    n, cin, h, w, cout, k, s, p = PATCH_SHAPE
    pb = patch_embed_problem()
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], "patch_embed7x7")
    out = torch.full(tuple(pb["ref"].shape), float("nan"), dtype=dtype, device=DEV)
    ops.conv_smallcin_kxk(pb["x"].to(DEV), pb["w"].to(DEV), pb["b"].to(DEV), out, k, s, p)
    L.assert_exact(out, pb["ref"], dtype, "patch_embed7x7", "nhwc")


DW_SHAPES = [(2, 64, 13, 17), (2, 64, 9, 3), (1, 128, 28, 30)]   # strip kernel (W >= 8), pixel-per-thread kernel (narrow), wider C


@functools.lru_cache(maxsize=3)
def dw_problem(shape):
    n, c, h, w = shape
    x = L.ints((n, c, h, w), -2, 2, 52)
    wt, b = L.weights((c, 1, 3, 3), 53), L.ints((c,), -8, 8, 54)
    assert _amax9(x) + 8 < L.EXACT_LIMIT
    ref = (F.conv2d(x.double(), wt.double(), b.double(), 1, 1, 1, c)).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=wt, b=b, ref=ref)


def _amax9(t):
    return 9.0 * float(t.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=["x".join(map(str, s)) for s in DW_SHAPES])
def test_dwconv3x3_exact(shape, dtype):
    ops = _ops()
    pb = dw_problem(shape)
    if dtype == BF:
        L.bf16_magnitude_ok(pb["ref"], f"dwconv {shape}")
    xv, _ = _to_nhwc_dev(pb["x"], dtype)
    out = torch.full(tuple(pb["ref"].shape), float("nan"), dtype=dtype, device=DEV)
    ops.dwconv3x3(xv.contiguous(), ops.pack_dwconv_weight(pb["w"].to(DEV)), pb["b"].to(DEV), out, act=ops.ACT_NONE)
    L.assert_exact(out, pb["ref"], dtype, f"dwconv3x3 {shape}", "nhwc")


def bf16_reference_cases():
    """(name, thunk -> float64 reference) of every bf16-output case of this file that must meet the magnitude condition; the host
    suite runs them all (tests/test_lattice_host.py), which also exercises every precondition assert of the ref64 wrappers."""
    cases = [(k, functools.partial(lambda k: fwd_problem(k)["ref"], k)) for k in FWD_TABLE]
    cases += [("splitk_" + s, functools.partial(lambda s: splitk_problem(s)["ref"], s)) for s in SPLITK_SHAPES]
    cases += [(f"cls{c}", functools.partial(lambda c: small_cout_problem(c)["ref"], c)) for c in SMALL_COUT]
    cases += [(f"epilogue_act{a}", functools.partial(lambda a: epilogue_problem(a)["ref"], a)) for a in EPI_ACTS]
    cases += [("res_rows", lambda: res_rows_problem()["ref"])]
    cases += [("linear_" + "x".join(map(str, s)), functools.partial(lambda s: linear_problem(s)["ref"], s)) for s in LINEAR_SHAPES]
    cases += [(f"stem3_{c}", functools.partial(lambda c: stem3_problem(c)["ref"], c)) for c in STEM3_CASES]
    cases += [("patch_embed", lambda: patch_embed_problem()["ref"])]
    cases += [(f"dw_{s}", functools.partial(lambda s: dw_problem(s)["ref"], s)) for s in DW_SHAPES]
    return cases
