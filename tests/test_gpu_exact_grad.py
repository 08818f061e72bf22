"""Bit-exact backward parity on integer-lattice inputs (tests/_lattice.py): data gradients, weight gradients (128 x 128 and 256 x 256
tiles, grouped launches, both destination layouts, accumulate / overwrite, split counts), the stem and depth-wise gradients, and the
reductions whose arithmetic is exact on integers, against float64 on the CPU - in the default (f32 atomics) mode and in deterministic
mode, which must therefore also equal each other.

Weight gradients are f32: products are integers of magnitude <= 4, so a sum over up to 4 M pixel rows is exact in any order and must be
torch.equal to the reference.  bf16 data gradients must equal ref.to(bfloat16).

Entry points held bit-exact here: cavp_conv2d_nhwc_aux as data gradient (stride 1 and the parity-ordered stride-2 tiles, residual
accumulation), cavp_pack_weight_dgrad, cavp_conv2d_wgrad_nhwc, cavp_conv2d_wgrad_group, cavp_set_wgrad_big (forced and automatic),
cavp_conv3x3_smallcin_wgrad, cavp_smallcin_kxk_im2col (+ the wgrad it feeds), cavp_dwconv3x3_bwd_data_nhwc, cavp_dwconv3x3_bwd,
cavp_colsum, cavp_colsum_groups, cavp_colstats (sum and sum of squares), cavp_global_avgpool_nhwc (HW a power of two),
cavp_bilinear_nhwc and cavp_bilinear_bwd_nhwc (x2, x4, align_corners=False: dyadic weights)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _lattice as L
from tests.test_gpu_train_ops import CONV, DEV
from tests.test_gpu_wgrad_big import BIG

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
DTYPES = [F32, BF]
IDS = ["f32", "bf16"]
SPLITS = [0, 1, 3, 7]
GRAD_TABLE = {c[0]: c for c in CONV}
GRAD_TABLE.update({"big_" + c[0]: c for c in BIG})


def _mods():
    from cavp_amd import _lib, ops, train_ops
    return _lib.load(), ops, train_ops


def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV)


def _seed(name, salt=0):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003 + 1000 * salt


@pytest.fixture(params=[False, True], ids=["atomics", "deterministic"])
def mode(request):
    """both reduction modes; deterministic goes through the suite's `deterministic` fixture"""
    if request.param:
        request.getfixturevalue("deterministic")
    return request.param


@pytest.fixture
def big():
    lib, _, _ = _mods()

    def set_(mode_, stagger=2):
        assert lib.cavp_set_wgrad_big(mode_, stagger) == 0
    yield set_
    assert lib.cavp_set_wgrad_big(0, 2) == 0


def grad_inputs(key):
    """lattice (x, w, dy, prev dx, prior dw OIHW, prior dbias) of one GRAD_TABLE case (cheap: no reference)"""
    name, n, h, w, cin, cout, k, s, p, d = GRAD_TABLE[key]
    ho, wo = (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1
    x = L.activations((n, cin, h, w), cin * k * k, _seed(key, 1))
    wt = L.weights((cout, cin, k, k), _seed(key, 2))
    dy = L.out_grads((n, cout, ho, wo), cout * k * k, _seed(key, 3))
    prev = L.ints((n, cin, h, w), -4, 4, _seed(key, 4))
    prior = L.ints((cout, cin, k, k), -3, 3, _seed(key, 5))
    pbias = L.ints((cout,), -3, 3, _seed(key, 6))
    return dict(x=x, w=wt, dy=dy, prev=prev, prior=prior, pbias=pbias, conv=(k, s, p, d))


@functools.lru_cache(maxsize=2)
def dgrad_problem(key):
    pb = grad_inputs(key)
    k, s, p, d = pb["conv"]
    pb["dx"] = L.ref64_dgrad(pb["dy"], pb["w"], pb["x"].shape, s, p, d).permute(0, 2, 3, 1).contiguous()
    pb["dx_acc"] = pb["dx"] + pb["prev"].double().permute(0, 2, 3, 1)
    return pb


@functools.lru_cache(maxsize=20)
def wgrad_problem(key):
    pb = grad_inputs(key)
    k, s, p, d = pb["conv"]
    pb["dw"], pb["db"] = L.ref64_wgrad(pb["x"], pb["dy"], pb["w"].shape, s, p, d)   # OIHW, [Cout]
    return pb


# ---- data gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("key", [c[0] for c in CONV])
def test_dgrad_exact(key, dt, mode):
    """every CONV case (pad <= dil * (k - 1) throughout), with and without a gradient already in the destination's residual input"""
    _, ops, T = _mods()
    pb = dgrad_problem(key)
    k, s, p, d = pb["conv"]
    assert p <= d * (k - 1)
    if dt == BF:
        L.bf16_magnitude_ok(pb["dx"], key + ".dgrad")
        L.bf16_magnitude_ok(pb["dx_acc"], key + ".dgrad+prev")
    dyv = _nhwc(pb["dy"], dt)
    wT = T.pack_weight_dgrad(pb["w"].to(DEV), dt)
    dx = torch.full(tuple(pb["dx"].shape), float("nan"), dtype=dt, device=DEV)
    T.conv2d_dgrad(dyv, wT, dx, kh=k, kw=k, stride=s, pad=p, dil=d)
    L.assert_exact(dx, pb["dx"], dt, key + ".dgrad", "nhwc")
    dx.fill_(float("nan"))
    T.conv2d_dgrad(dyv, wT, dx, kh=k, kw=k, stride=s, pad=p, dil=d, residual=_nhwc(pb["prev"], dt))
    L.assert_exact(dx, pb["dx_acc"], dt, key + ".dgrad+prev", "nhwc")


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
def _wgrad_all_plans(T, pb, key, dt, tag):
    """both layouts x accumulate / overwrite x split counts, dbias accumulating throughout"""
    k, s, p, d = pb["conv"]
    xv, dyv = _nhwc(pb["x"], dt), _nhwc(pb["dy"], dt)
    prior = pb["prior"].double()
    for sk in SPLITS:
        for oihw in (False, True):
            for over in (False, True):
                start = pb["prior"] if oihw else pb["prior"].permute(0, 2, 3, 1).contiguous()
                dw = (torch.full_like(start, 7.5) if over else start.clone()).to(DEV)
                db = pb["pbias"].clone().to(DEV)
                T.conv2d_wgrad(xv, dyv, dw, kh=k, kw=k, stride=s, pad=p, dil=d, dw_oihw=oihw, splitk=sk, overwrite=over, dbias=db)
                want = pb["dw"] if over else pb["dw"] + prior
                what = f"{key}.{tag}.sk{sk}.{'oihw' if oihw else 'ohwi'}.{'overwrite' if over else 'accumulate'}"
                L.assert_exact(dw if oihw else dw.permute(0, 3, 1, 2), want, F32, what, ("o", "i", "kh", "kw"))
                L.assert_exact(db, pb["db"] + pb["pbias"].double(), F32, what + ".dbias", ("o",))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("key", [c[0] for c in CONV])
def test_wgrad_exact(key, dt, mode):
    _, ops, T = _mods()
    _wgrad_all_plans(T, wgrad_problem(key), key, dt, "small_tile")


@pytest.mark.parametrize("stagger", [2, 1, 0], ids=["16waves", "8waves_interleaved", "8waves_plain"])
@pytest.mark.parametrize("key", [c[0] for c in CONV])
def test_wgrad_big_tile_forced_exact(key, stagger, big, mode):
    """the 256 x 256 tile forced onto every small shape: dead 32-channel blocks, pixel ranges shorter than one ring trip"""
    _, ops, T = _mods()
    big(2, stagger)
    _wgrad_all_plans(T, wgrad_problem(key), key, BF, f"big_tile.stagger{stagger}")


@pytest.mark.parametrize("key", ["big_" + c[0] for c in BIG])
def test_wgrad_big_tile_auto_exact(key, big):
    """>= 16384 pixel rows: the automatic choice of the 256 x 256 tile in its three schedules, and the 128 x 128 tile on the same
    inputs - all four must be THE gradient (the tolerance test allowed ~7 absolute on head0_like)"""
    _, ops, T = _mods()
    pb = wgrad_problem(key)
    k, s, p, d = pb["conv"]
    cout, cin = pb["w"].shape[:2]
    xv, dyv = _nhwc(pb["x"], BF), _nhwc(pb["dy"], BF)
    for mode_, stagger in ((0, 2), (0, 1), (0, 0), (1, 1)):
        big(mode_, stagger)
        dw = pb["prior"].permute(0, 2, 3, 1).contiguous().to(DEV)
        db = pb["pbias"].clone().to(DEV)
        T.conv2d_wgrad(xv, dyv, dw, kh=k, kw=k, stride=s, pad=p, dil=d, dbias=db)
        what = f"{key}.mode{mode_}.stagger{stagger}"
        L.assert_exact(dw.permute(0, 3, 1, 2), pb["dw"] + pb["prior"].double(), F32, what, ("o", "i", "kh", "kw"))
        L.assert_exact(db, pb["db"] + pb["pbias"].double(), F32, what + ".dbias", ("o",))


GROUP_KEYS = ["big_" + BIG[0][0], CONV[0][0], "big_" + BIG[1][0], CONV[8][0], CONV[2][0], CONV[11][0], CONV[12][0], CONV[10][0]]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_wgrad_group_exact(dt, big, mode):
    """one grouped launch that mixes jobs of both tiles (bf16), layouts, accumulate / overwrite, bias / no bias and split counts"""
    _, ops, T = _mods()
    big(0, 2)
    jobs, refs = [], []
    for i, key in enumerate(GROUP_KEYS):
        pb = wgrad_problem(key)
        k, s, p, d = pb["conv"]
        oihw, over, bias = bool(i & 1), bool(i & 2), i % 3 != 1
        start = pb["prior"] if oihw else pb["prior"].permute(0, 2, 3, 1).contiguous()
        dw = (torch.full_like(start, 7.5) if over else start.clone()).to(DEV)
        db = pb["pbias"].clone().to(DEV) if bias else None
        jobs.append(dict(x=_nhwc(pb["x"], dt), dy=_nhwc(pb["dy"], dt), dw=dw, kh=k, kw=k, stride=s, pad=p, dil=d, dbias=db,
                         dw_oihw=oihw, overwrite=over, splitk=(5, 1, 7, 3, 2, 0, 0, 1)[i]))
        refs.append((key, pb["dw"] if over else pb["dw"] + pb["prior"].double(), pb["db"] + pb["pbias"].double()))
    T.conv2d_wgrad_group(jobs)
    for j, (key, want, wantb) in zip(jobs, refs):
        L.assert_exact(j["dw"] if j["dw_oihw"] else j["dw"].permute(0, 3, 1, 2), want, F32, key + ".group", ("o", "i", "kh", "kw"))
        if j["dbias"] is not None:
            L.assert_exact(j["dbias"], wantb, F32, key + ".group.dbias", ("o",))


LINEAR_WGRAD = [(6272, 304, 1216), (64, 4096, 304), (4, 12288, 512), (6272, 256, 304)]


def linear_wgrad_inputs(shape):
    rows, cin, cout = shape
    return L.activations((rows, cin), cin, 5), L.out_grads((rows, cout), cout, 6)


@functools.lru_cache(maxsize=1)
def linear_wgrad_problem(shape):
    x, dy = linear_wgrad_inputs(shape)
    dw, db = L.ref64_linear_wgrad(x, dy)
    return dict(x=x, dy=dy, dw=dw, db=db)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", LINEAR_WGRAD, ids=["x".join(map(str, s)) for s in LINEAR_WGRAD])
def test_linear_wgrad_exact(shape, dt, mode):
    _, ops, T = _mods()
    rows, cin, cout = shape
    pb = linear_wgrad_problem(shape)
    prior, pbias = L.ints((cout, cin), -3, 3, 7), L.ints((cout,), -3, 3, 8)
    dw, db = prior.clone().to(DEV), pbias.clone().to(DEV)
    T.linear_wgrad(pb["x"].to(dt).to(DEV), pb["dy"].to(dt).to(DEV), dw, dbias=db)
    L.assert_exact(dw, pb["dw"] + prior.double(), F32, f"linear_wgrad {shape}", ("o", "i"))
    L.assert_exact(db, pb["db"] + pbias.double(), F32, f"linear_wgrad {shape}.dbias", ("o",))


# ---- stems and PVT pieces -----------------------------------------------------------------------------------------------------------
STEM3_WGRAD = [(3, 2, (32, 40)), (1, 1, (24, 16)), (3, 2, (31, 45)), (2, 1, (9, 300)), (3, 2, (224, 224))]


def stem3_wgrad_inputs(case):
    cin, stride, hw = case
    ho, wo = (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1
    return L.ints((2, cin, *hw), -2, 2, 34), L.ints((2, 64, ho, wo), -2, 2, 36)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", STEM3_WGRAD, ids=[f"cin{c}-s{s}-{h}x{w}" for c, s, (h, w) in STEM3_WGRAD])
def test_smallcin_wgrad_exact(case, dt):
    """(bf16 / 64 channels = the fused matrix-core kernel; f32 = the im2col + GEMM route); accumulates onto an integer gradient"""
    _, ops, T = _mods()
    cin, stride, hw = case
    x, dy = stem3_wgrad_inputs(case)
    prior = L.ints((64, cin, 3, 3), -3, 3, 37)
    want, _ = L.ref64_wgrad(x, dy, (64, cin, 3, 3), stride, 1, 1, prior=prior)
    dw = prior.clone().to(DEV)
    T.smallcin_wgrad(x.to(DEV), _nhwc(dy, dt), dw, stride)
    L.assert_exact(dw, want, F32, f"smallcin wgrad {case}", ("o", "i", "kh", "kw"))


PATCH_SHAPE = (2, 3, 64, 96, 64, 7, 4, 3)   # N, Cin, H, W, Cout, k, stride, pad


def patch_wgrad_inputs():
    n, cin, h, w, cout, k, s, p = PATCH_SHAPE
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return L.ints((n, cin, h, w), -2, 2, 55), L.ints((n, cout, ho, wo), -2, 2, 58)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_conv_smallcin_kxk_wgrad_exact(dt):
    _, ops, T = _mods()
    n, cin, h, w, cout, k, s, p = PATCH_SHAPE
    x, dy = patch_wgrad_inputs()
    prior = L.ints((cout, cin, k, k), -3, 3, 59)
    want, _ = L.ref64_wgrad(x, dy, (cout, cin, k, k), s, p, 1, prior=prior)
    dw = prior.clone().to(DEV)
    T.conv_smallcin_kxk_wgrad(x.to(DEV), _nhwc(dy, dt), dw, k, s, p)
    L.assert_exact(dw, want, F32, "patch_embed7x7 wgrad", ("o", "i", "kh", "kw"))


DW_SHAPES = [(2, 64, 13, 17), (2, 64, 9, 3), (3, 128, 28, 30)]


@functools.lru_cache(maxsize=3)
def dw_grad_problem(shape):
    n, c, h, w = shape
    x = L.ints((n, c, h, w), -2, 2, 52).double().requires_grad_(True)
    wt = L.weights((c, 1, 3, 3), 53).double().requires_grad_(True)
    dy = L.ints((n, c, h, w), -2, 2, 61)
    assert n * h * w * 4 + 3 < L.EXACT_LIMIT
    F.conv2d(x, wt, None, 1, 1, 1, c).backward(dy.double())
    return dict(x=x.detach().float(), w=wt.detach().float(), dy=dy, dx=x.grad.permute(0, 2, 3, 1).contiguous(), dw=wt.grad,
                db=dy.double().sum((0, 2, 3)))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", DW_SHAPES, ids=["x".join(map(str, s)) for s in DW_SHAPES])
def test_dwconv3x3_grads_exact(shape, dt, mode):
    """data gradient from the forward's packed taps, the weight / bias gradient alone, and both in one walk over dy"""
    _, ops, T = _mods()
    n, c, h, w = shape
    pb = dw_grad_problem(shape)
    if dt == BF:
        L.bf16_magnitude_ok(pb["dx"], f"dwconv dx {shape}")
    xv, dyv = _nhwc(pb["x"], dt), _nhwc(pb["dy"], dt)
    w9c = ops.pack_dwconv_weight(pb["w"].to(DEV))
    dx = torch.full((n, h, w, c), float("nan"), dtype=dt, device=DEV)
    ops.dwconv3x3_bwd_data(dyv, w9c, dx)
    L.assert_exact(dx, pb["dx"], dt, f"dwconv3x3 data gradient {shape}", "nhwc")
    prior, pbias = L.ints((c, 1, 3, 3), -3, 3, 62), L.ints((c,), -3, 3, 63)
    for fused in (False, True):
        dw, db = prior.clone().to(DEV), pbias.clone().to(DEV)
        dx2 = torch.full((n, h, w, c), float("nan"), dtype=dt, device=DEV) if fused else None
        T.dwconv3x3_wgrad(xv, dyv, dw, db, w9c=w9c if fused else None, dx=dx2)
        L.assert_exact(dw, pb["dw"] + prior.double(), F32, f"dwconv3x3 wgrad {shape} fused={fused}", ("c", "one", "kh", "kw"))
        L.assert_exact(db, pb["db"] + pbias.double(), F32, f"dwconv3x3 dbias {shape} fused={fused}", ("c",))
        if fused:
            L.assert_exact(dx2, pb["dx"], dt, f"dwconv3x3 fused data gradient {shape}", "nhwc")


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,C", [(333, 304), (6272, 256), (5, 64), (20000, 48)])
def test_colsum_and_colstats_exact(rows, C, dt, mode):
    _, ops, T = _mods()
    x = L.ints((rows, C), -2, 2, 14)
    assert rows * 4 + 3 < L.EXACT_LIMIT
    prior = L.ints((C,), -3, 3, 15)
    cs = prior.clone().to(DEV)
    T.colsum(x.to(dt).to(DEV), cs)
    L.assert_exact(cs, x.double().sum(0) + prior.double(), F32, "colsum", ("c",))
    sums, sq = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    T.colstats(x.to(dt).to(DEV), sums, sq)
    L.assert_exact(sums, x.double().sum(0), F32, "colstats.sum", ("c",))
    L.assert_exact(sq, (x.double() ** 2).sum(0), F32, "colstats.sumsq", ("c",))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_colsum_groups_exact(dt, mode):
    """per-image column sums of a channel slice, accumulating"""
    _, ops, T = _mods()
    G, H, W, C = 5, 14, 13, 256
    x = L.ints((G, H, W, C + 16), -2, 2, 40)
    prior = L.ints((G, C), -3, 3, 41)
    out = prior.clone().to(DEV)
    T.colsum_groups(x.to(dt).to(DEV)[..., 8:8 + C], out)
    L.assert_exact(out, x[..., 8:8 + C].double().sum((1, 2)) + prior.double(), F32, "colsum_groups", ("g", "c"))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(16, 16), (8, 4), (1, 1), (32, 64)])
def test_global_avgpool_exact(hw, dt):
    """HW a power of two: sum / HW (or sum * (1 / HW)) is exact"""
    _, ops, T = _mods()
    x = L.ints((3, 200, *hw), -2, 2, 23)
    buf = torch.full((3, *hw, 208), 7.0, dtype=dt, device=DEV)
    buf[..., 8:208] = _nhwc(x, dt)
    out = torch.full((3, 200), float("nan"), dtype=F32, device=DEV)
    ops.global_avgpool(buf[..., 8:208], out)
    L.assert_exact(out, x.double().flatten(2).mean(-1), F32, f"global_avgpool {hw}", ("n", "c"))


BILINEAR = [((14, 14), 2), ((14, 14), 4), ((7, 9), 2), ((7, 9), 4), ((1, 1), 4), ((28, 28), 2)]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("hi,up", BILINEAR, ids=[f"{h}x{w}-x{u}" for (h, w), u in BILINEAR])
def test_bilinear_fwd_bwd_exact(hi, up, dt):
    """align_corners=False at x2 / x4: the interpolation weights are k/4 resp. k/8 per axis, so every output is an integer / 64 -
    exact in f32, and at most 8 significant bits (exact in bf16) in the forward.  The backward sums up to 64 such terms: exact in
    f32, rounded once for bf16."""
    _, ops, T = _mods()
    ho = (hi[0] * up, hi[1] * up)
    x = L.ints((2, 32, *hi), -2, 2, 24).double().requires_grad_(True)
    y = F.interpolate(x, size=ho, mode="bilinear", align_corners=False)
    dy = L.ints(tuple(y.shape), -2, 2, 28)
    y.backward(dy.double())
    assert bool(((y.detach() * 64) == (y.detach() * 64).round()).all()) and bool(((x.grad * 64) == (x.grad * 64).round()).all())
    big = torch.zeros((2, ho[0], ho[1], 48), dtype=dt, device=DEV)
    ops.bilinear(_nhwc(x.detach().float(), dt), big[..., :32], False)
    L.assert_exact(big[..., :32], y.detach().permute(0, 2, 3, 1), dt, f"bilinear {hi} x{up}", "nhwc")
    assert float(big[..., 32:].float().abs().max()) == 0.0, "wrote outside its channel slice"
    big[..., :32] = _nhwc(dy, dt)
    dx = torch.full((2, hi[0], hi[1], 32), float("nan"), dtype=dt, device=DEV)
    T.bilinear_bwd(big[..., :32], dx, False)
    L.assert_exact(dx, x.grad.permute(0, 2, 3, 1), dt, f"bilinear_bwd {hi} x{up}", "nhwc")


def bf16_reference_cases():
    """(name, thunk -> float64 reference) of the bf16-output cases of this file that must meet the magnitude condition"""
    cases = []
    for c in CONV:
        cases.append((c[0] + ".dgrad", functools.partial(lambda k: dgrad_problem(k)["dx"], c[0])))
        cases.append((c[0] + ".dgrad+prev", functools.partial(lambda k: dgrad_problem(k)["dx_acc"], c[0])))
    cases += [(f"dw_dx_{s}", functools.partial(lambda s: dw_grad_problem(s)["dx"], s)) for s in DW_SHAPES]
    return cases


def wgrad_input_cases():
    """(name, thunk -> (x, dy, pixel rows)) of every f32-output weight-gradient case: the host suite checks ranges and rows * 4 < 2^24"""
    def conv(key):
        pb = grad_inputs(key)
        return pb["x"], pb["dy"], pb["dy"].numel() // pb["dy"].shape[1]
    cases = [(k, functools.partial(conv, k)) for k in GRAD_TABLE]
    cases += [("linear_" + "x".join(map(str, s)), functools.partial(lambda s: linear_wgrad_inputs(s) + (s[0],), s)) for s in LINEAR_WGRAD]
    cases += [(f"stem3_{c}", functools.partial(lambda c: (lambda x, dy: (x, dy, dy.numel() // 64))(*stem3_wgrad_inputs(c)), c))
              for c in STEM3_WGRAD]
    cases += [("patch_embed", lambda: (lambda x, dy: (x, dy, dy.numel() // PATCH_SHAPE[4]))(*patch_wgrad_inputs()))]
    return cases
