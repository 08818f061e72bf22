"""The implicit-GEMM conv (csrc/conv_igemm.hip) on launches larger than its persistent grid.

launch_cfg launches at most 4 x 256 workgroups; a launch with more tiles than that has every workgroup walk `vb += gridDim.x`, and
between two tiles it runs the loop tail: start_tile() of the next tile re-derives the split-K slice, the channel and pixel tile, the
rotated parity class of a stride-2 data gradient, the K range, the BatchNorm-backward coefficients, and issues the next tile's first
ring stages behind the previous tile's stores.  Every launch here has at least 2049 logical workgroups - more than twice the largest
grid - so every physical workgroup walks at least two tiles whatever the occupancy query returns.

Outputs are prefilled with NaN (an element that no tile writes fails the finiteness check) and compared with float64 CPU references of
the same operation on storage-rounded operands, computed once per (shape, dtype) and shared by all tiles.  Tile 10 (the 256 x 256
tile, its own kernel) is covered in test_gpu_igemm_big.py."""
import ctypes as C
import os
import re
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_ops import DEV, _check, _q, _rand
from tests.test_gpu_train_ops import _check as _check_grad

gpu = pytest.mark.gpu
NAN = float("nan")
BF = torch.bfloat16
DTYPES = [torch.float32, BF]

# kTiles[] and tile_stages() of conv_igemm.hip: id -> (BC output channels, BP output pixels, ring stages).
# test_ktiles_mirror_matches_the_kernel_source fails when the two drift apart.
KTILES = {1: (128, 128, 2), 2: (64, 128, 2), 3: (64, 64, 2), 4: (128, 64, 2), 5: (128, 32, 2), 6: (16, 128, 2), 7: (32, 128, 2),
          8: (256, 128, 3), 9: (128, 256, 3), 10: (256, 256, 2), 11: (64, 64, 4), 12: (64, 64, 8), 13: (128, 64, 4),
          14: (64, 128, 4)}
TILES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14]
RING_TILES = [t for t in TILES if KTILES[t][2] > 2]   # 3-, 4- and 8-stage rings: start_tile issues NS-1 stages, some of them fill
BNB_TILES = [1, 2, 3, 4, 11, 13, 14]                 # tile_has_bnb
MAX_GRID = 4 * 256                                   # launch_cfg: at most 4 resident workgroups per CU, 256 CUs
MIN_WG = 2 * MAX_GRID + 1


def _cdiv(a, b):
    return -(-a // b)


def _wg(tile, rows, cout, splitk=1):
    """logical workgroups of a launch (make_plan: nblk)."""
    bc, bp, _ = KTILES[tile]
    return _cdiv(cout, bc) * _cdiv(rows, bp) * splitk


def _par_rows(n, h, w, tile):
    """pixel rows of a parity-ordered stride-2 data gradient (make_plan: four classes, each padded to the tile height)."""
    bp = KTILES[tile][1]
    return 4 * _cdiv(n * _cdiv(h, 2) * _cdiv(w, 2), bp) * bp


def _out_hw(h, w, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# one float64 reference per (shape, dtype); the parametrizations below keep the tile innermost, so a small LRU suffices
_CACHE = OrderedDict()


def _cached(key, make, keep=2):
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    while len(_CACHE) >= keep:
        _CACHE.popitem(last=False)
    _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# forward cases: 200 output channels (a partial last channel tile for every tile), ~270 k output pixels (tiles 8 and 9 are the
# tightest at ~2110 workgroups)
# ---------------------------------------------------------------------------------------------------------------------------
# name: (N, H, W, Cin f32, Cin bf16, k, stride, pad, dil, tiles, epilogue)
FWD = {
    # one K iteration (bf16 Cin 64, f32 Cin 32): every tile boundary is also a K boundary
    "1x1_k1": (4, 257, 263, 32, 64, 1, 1, 0, 1, TILES, False),
    # 3x3 pad 1 on a ragged image: the last pixel tile is partial, pixel tiles cross image rows and images, K tails (Cin 16)
    "3x3_ragged": (4, 257, 263, 16, 16, 3, 1, 1, 1, TILES, False),
    # K loops shorter than the ring: 2 and 3 K iterations (start_tile's fill DMAs, gdma(s, s < n))
    "1x1_k2": (4, 257, 263, 64, 128, 1, 1, 0, 1, RING_TILES, False),
    "1x1_k3": (4, 257, 263, 96, 192, 1, 1, 0, 1, RING_TILES, False),
    # stride 2 (513 x 525 -> 257 x 263)
    "3x3_s2": (4, 513, 525, 8, 8, 3, 2, 1, 1, TILES, False),
    # dilation 16 on 14 x 20 images: 6 of the 9 taps are dead (removed on the host), the 3 live ones are out of the image for most
    # pixels; 280-pixel images, so every pixel tile crosses images
    "3x3_d16_deadtaps": (966, 14, 20, 16, 16, 3, 1, 16, 16, TILES, False),
    # the full epilogue: scale, shift, residual, activation
    "1x1_k1_epilogue": (4, 257, 263, 32, 64, 1, 1, 0, 1, TILES, True),
}
COUT = 200


def _fwd_ref(name, dtype):
    def make():
        n, h, w, cf, cb, k, s, p, d, _, epi = FWD[name]
        cin = cf if dtype == torch.float32 else cb
        x = _q(_rand(n, cin, h, w, seed=101) + 0.25, dtype)
        wt = _q(_rand(COUT, cin, k, k, seed=102, scale=(cin * k * k) ** -0.5), dtype)
        ref = F.conv2d(x.double(), wt.double(), None, s, p, d)
        from cavp_amd import ops
        e = dict(xv=_nhwc(x, dtype), wp=ops.pack_weight(wt.to(DEV), dtype))
        if epi:
            sc = torch.rand(COUT, generator=torch.Generator().manual_seed(103)) + 0.5
            sh = _rand(COUT, seed=104)
            res = _q(_rand(n, COUT, ref.shape[2], ref.shape[3], seed=105), dtype)
            ref = ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None] + res.double()
            ref = F.leaky_relu(ref, 0.01)
            e.update(sc=sc.to(DEV), sh=sh.to(DEV), rv=_nhwc(res, dtype))
        e["ref"] = ref.permute(0, 2, 3, 1).contiguous()
        return e
    return _cached(("fwd", name, dtype), make)


def _fwd_launch(name, dtype, tile, e, out, **kw):
    from cavp_amd import ops
    n, h, w, cf, cb, k, s, p, d, _, epi = FWD[name]
    if epi:
        kw.update(scale=e["sc"], shift=e["sh"], residual=e["rv"], act=ops.ACT_LEAKY)
    return ops.conv2d(e["xv"], e["wp"], out, kh=k, kw=k, stride=s, pad=p, dil=d, tile=tile, **kw)


def _fwd_rows(name):
    n, h, w, cf, cb, k, s, p, d, _, _ = FWD[name]
    ho, wo = _out_hw(h, w, k, s, p, d)
    return n * ho * wo, ho, wo


FWD_PARAMS = [pytest.param(name, dt, t, id=f"{name}-{'f32' if dt == torch.float32 else 'bf16'}-tile{t}")
              for name in FWD for dt in DTYPES for t in FWD[name][9]]

# forced split-K (the planner keeps a split only where iters >= 4 * splitk): 3x3 Cin 128 = 18 (bf16) / 36 (f32) K iterations
SPLITK_CASE = (4, 70, 70, 128, 3, 1, 1, 1)   # N, H, W, Cin, k, stride, pad, dil
SPLITK_TILES = [3, 11]

# data gradients of a forward conv 200 -> 16 channels: dx has 200 channels and ~270 k pixels (stride 2: in four parity classes)
# name: (N, H, W (of dx), k, stride, pad)
DGRAD = {
    "3x3_s1": (4, 257, 263, 3, 1, 1),
    "3x3_s2_odd": (4, 257, 263, 3, 2, 1),   # classes of 4, 2, 2 and 1 taps, of different sizes
    "1x1_s2": (4, 257, 263, 1, 2, 0),       # three of the four classes have no tap: tiles without a K loop
}
DG_COF = 16   # forward output channels = K of the data gradient (one K iteration per tap)
BNB_N = 2     # the fused BatchNorm-backward cases run on the first two images (the 128 x 128 tile still has > 2048 workgroups)
BNB_CASES = [("3x3_s1", False), ("3x3_s1", True), ("1x1_s2", True), ("3x3_s2_odd", False)]


def _dgrad_rows(name, tile, n=None):
    n0, h, w, k, s, p = DGRAD[name]
    n = n or n0
    return _par_rows(n, h, w, tile) if s == 2 else n * h * w


def _all_launches():
    """(what, workgroups) of every launch in this file."""
    out = []
    for name, (n, h, w, cf, cb, k, s, p, d, tiles, _) in FWD.items():
        for t in tiles:
            out.append((f"fwd {name} tile {t}", _wg(t, _fwd_rows(name)[0], COUT)))
    n, h, w, cin, k, s, p, d = SPLITK_CASE
    for t in SPLITK_TILES:
        for sk in (2, 3):
            out.append((f"splitk {sk} tile {t}", _wg(t, n * h * w, COUT, sk)))
    for name in DGRAD:
        for t in TILES:
            out.append((f"dgrad {name} tile {t}", _wg(t, _dgrad_rows(name, t), COUT)))
    for name, _ in BNB_CASES:
        for t in BNB_TILES:
            out.append((f"bnb {name} tile {t}", _wg(t, _dgrad_rows(name, t, BNB_N), COUT)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# CPU checks: the mirror and the premise
# ---------------------------------------------------------------------------------------------------------------------------
def test_ktiles_mirror_matches_the_kernel_source():
    """KTILES above == the kTiles[] initialiser, tile_stages() and the launch_tile instantiations of conv_igemm.hip."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cavp_amd", "csrc",
                            "conv_igemm.hip")).read()
    body = re.search(r"const TileCfg kTiles\[\] = \{(.*?)\n\};", src, re.S)
    assert body, "kTiles[] initialiser not found"
    text = re.sub(r"//[^\n]*", "", body.group(1))
    entries = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*[0-9.]+f?\s*\}", text)
    assert len(entries) == text.count("{"), "unparsed kTiles[] entries"
    geom = {int(i): (int(bc), int(bp)) for i, bc, bp in entries}
    stages_expr = re.search(r"inline int tile_stages\(int id\) \{ return (.*?); \}", src)
    assert stages_expr, "tile_stages() not found"
    expr = stages_expr.group(1)
    arms = re.findall(r"id\s*(==|>=|<=|>|<)\s*(\d+)\s*\?\s*(\d+)\s*:\s*", expr)
    default = re.fullmatch(r"(?:id\s*(?:==|>=|<=|>|<)\s*\d+\s*\?\s*\d+\s*:\s*)+(\d+)", expr)
    assert arms and default, f"tile_stages() is no longer a chain of `id <op> N ? S :` arms: {expr}"
    ops_ = {"==": int.__eq__, ">=": int.__ge__, "<=": int.__le__, ">": int.__gt__, "<": int.__lt__}

    def stages(i):
        for op, v, st in arms:
            if ops_[op](i, int(v)):
                return int(st)
        return int(default.group(1))
    src_tiles = {i: (bc, bp, stages(i)) for i, (bc, bp) in geom.items()}
    assert src_tiles == KTILES
    # the kernels launch_tile instantiates have the geometry the planner counts workgroups with
    plain = re.search(r"hipError_t launch_tile\(int id.*?\n  switch \(id\) \{(.*?)\n  \}", src, re.S)
    assert plain, "launch_tile's switch not found"
    for i, bc, bp, ns in re.findall(r"case (\d+): return launch_cfg<T, (\d+), (\d+), \d+, \d+, UP(?:, (\d+))?>", plain.group(1)):
        assert (int(bc), int(bp), int(ns or 2)) == KTILES[int(i)], f"launch_tile case {i}"
    assert sorted(TILES + [10]) == sorted(KTILES)
    assert re.search(r"inline bool tile_has_bnb\(int id\) \{ return (.*?); \}", src).group(1) == \
        " || ".join(f"id == {t}" for t in BNB_TILES)


def test_every_launch_walks_at_least_two_tiles_per_workgroup():
    """each launch of this file has more than twice as many workgroups as the largest persistent grid."""
    short = [(what, n) for what, n in _all_launches() if n < MIN_WG]
    assert not short, short


# ---------------------------------------------------------------------------------------------------------------------------
# a. forward, forced tiles
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,dtype,tile", FWD_PARAMS)
def test_forward_forced_tile(name, dtype, tile):
    rows, ho, wo = _fwd_rows(name)
    assert _wg(tile, rows, COUT) >= MIN_WG
    e = _fwd_ref(name, dtype)
    out = _nan((FWD[name][0], ho, wo, COUT), dtype)
    _fwd_launch(name, dtype, tile, e, out)
    _check(out, e["ref"], dtype, f"{name}/tile{tile}")


# ---------------------------------------------------------------------------------------------------------------------------
# b. forced split-K across trips: a workgroup changes its K slice z between tiles
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("splitk", [2, 3])
@pytest.mark.parametrize("tile", SPLITK_TILES)
def test_forward_splitk_across_trips(tile, splitk, dtype):
    from cavp_amd import _lib, ops
    n, h, w, cin, k, s, p, d = SPLITK_CASE
    assert _wg(tile, n * h * w, COUT, splitk) >= MIN_WG

    def make():
        x = _q(_rand(n, cin, h, w, seed=111), dtype)
        wt = _q(_rand(COUT, cin, k, k, seed=112, scale=(cin * k * k) ** -0.5), dtype)
        ref = F.conv2d(x.double(), wt.double(), None, s, p, d)
        return dict(xv=_nhwc(x, dtype), wp=ops.pack_weight(wt.to(DEV), dtype), ref=ref.permute(0, 2, 3, 1).contiguous())
    e = _cached(("splitk", dtype), make)
    desc = _lib.ConvDesc(dtype=ops.dtype_code(dtype), N=n, H=h, W=w, Cin=cin, ldx=cin, Cout=COUT, ldy=COUT, KH=k, KW=k, stride=s,
                         pad=p, dil=d, splitk=splitk, tile=tile)
    nbytes = _lib.load().cavp_conv2d_workspace_bytes(C.byref(desc))
    assert nbytes == splitk * n * h * w * COUT * 4, "the plan did not split K as asked"
    # the slabs are written, not accumulated: poison them too, so that a slab no tile writes cannot pass with an earlier launch's
    ops.workspace(nbytes, DEV)[:nbytes].view(torch.float32).fill_(NAN)
    out = _nan((n, h, w, COUT), dtype)
    ops.conv2d(e["xv"], e["wp"], out, kh=k, kw=k, stride=s, pad=p, dil=d, splitk=splitk, tile=tile)
    _check(out, e["ref"], dtype, f"splitk{splitk}/tile{tile}")


# ---------------------------------------------------------------------------------------------------------------------------
# c. forward fused BatchNorm statistics across trips
# ---------------------------------------------------------------------------------------------------------------------------
STATS_CASE = "3x3_ragged"


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("tile", TILES)
def test_forward_tile_statistics_across_trips(tile, dtype):
    """per-tile (mean, M2) from the epilogue == float64 per pixel tile, and bn_finalize_tiles' mean / rstd == float64.
    The weights are scaled by a power of two unique to (tile, dtype) - exact in bf16, so the reference is the shared one scaled -
    which makes a statistics slot that no tile writes fail even when the caching allocator hands back the buffer of an earlier launch
    (ops.conv2d allocates it uninitialised)."""
    from cavp_amd import ops, train_ops as T
    rows, ho, wo = _fwd_rows(STATS_CASE)
    assert _wg(tile, rows, COUT) >= MIN_WG
    n = FWD[STATS_CASE][0]
    e = _fwd_ref(STATS_CASE, dtype)
    f = 2.0 ** (TILES.index(tile) + len(TILES) * DTYPES.index(dtype))
    out = _nan((n, ho, wo, COUT), dtype)
    out, stats = ops.conv2d(e["xv"], e["wp"] * f, out, kh=3, kw=3, pad=1, splitk=1, tile=tile, want_tile_stats=True)
    assert stats is not None, "a forced unsplit 4- / 8-wave tile carries the fused statistics"
    ts, tiles, rpt = stats
    bp = KTILES[tile][1]
    assert (tiles, rpt) == (_cdiv(rows, bp), bp)
    ref = e["ref"].view(rows, COUT) * f
    _check(out.view(rows, COUT), ref, dtype, f"stats launch output/tile{tile}")
    # per pixel tile, float64
    full = rows // bp
    cnt = torch.full((tiles, 1), float(bp), dtype=torch.float64)
    cnt[-1] = rows - (tiles - 1) * bp
    s1 = torch.cat([ref[:full * bp].view(full, bp, COUT).sum(1), ref[full * bp:].sum(0, keepdim=True)])
    s2 = torch.cat([(ref[:full * bp] ** 2).view(full, bp, COUT).sum(1), (ref[full * bp:] ** 2).sum(0, keepdim=True)])
    t_mean = s1 / cnt
    t_var = s2 / cnt - t_mean ** 2
    got = ts.cpu().double()
    assert torch.isfinite(got).all(), "a statistics slot was not written"
    zmax = float(ref.abs().max())
    err_m = float((got[:, :, 0] - t_mean).abs().max())
    err_v = float((got[:, :, 1] / cnt - t_var).abs().max())
    assert err_m <= 2e-5 * zmax, f"tile means: {err_m:.3e} (|z| max {zmax:.3g})"
    assert err_v <= 1e-4 * zmax ** 2, f"tile variances: {err_v:.3e} (|z| max {zmax:.3g})"
    # finalized over all tiles
    g, b = torch.ones(COUT, device=DEV), torch.zeros(COUT, device=DEV)
    mk = lambda: torch.full((COUT,), NAN, device=DEV)   # noqa: E731
    scale, shift, mean, rstd = mk(), mk(), mk(), mk()
    T.bn_finalize_tiles(ts, tiles, rpt, rows, g, b, 1e-5, 0.1, None, None, scale, shift, mean, rstd)
    m_ref, v_ref = ref.mean(0), ref.var(0, unbiased=False)
    _check_grad(mean, m_ref, torch.float32, "mean", 2e-5)
    _check_grad(rstd, 1 / torch.sqrt(v_ref + 1e-5), torch.float32, "rstd", 5e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# d. data gradients, forced tiles (stride 2: parity-ordered tiles, class rotated per trip)
# ---------------------------------------------------------------------------------------------------------------------------
def _dgrad_ref(name, dtype):
    def make():
        from cavp_amd import train_ops as T
        n, h, w, k, s, p = DGRAD[name]
        ho, wo = _out_hw(h, w, k, s, p, 1)
        wt = _q(_rand(DG_COF, COUT, k, k, seed=121, scale=(COUT * k * k) ** -0.5), dtype)   # forward weight: 200 -> 16
        dy = _q(_rand(n, DG_COF, ho, wo, seed=122), dtype)
        prev = _q(_rand(n, COUT, h, w, seed=123) * 0.5, dtype)
        # float64 autograd's data gradient, one image at a time (the CPU transposed conv unfolds a large column buffer per image)
        dx = torch.cat([torch.nn.grad.conv2d_input((1, COUT, h, w), wt.double(), dy[i:i + 1].double(), s, p, 1) for i in range(n)])
        return dict(dyv=_nhwc(dy, dtype), wT=T.pack_weight_dgrad(wt.to(DEV), dtype), prev=prev, prevv=_nhwc(prev, dtype),
                    dx=dx.permute(0, 2, 3, 1).contiguous(), prev_nhwc=prev.permute(0, 2, 3, 1).contiguous())
    return _cached(("dgrad", name, dtype), make)


DGRAD_PARAMS = [pytest.param(name, dt, t, id=f"{name}-{'f32' if dt == torch.float32 else 'bf16'}-tile{t}")
                for name in DGRAD for dt in DTYPES for t in TILES]


@gpu
@pytest.mark.parametrize("name,dtype,tile", DGRAD_PARAMS)
def test_dgrad_forced_tile(name, dtype, tile):
    from cavp_amd import train_ops as T
    n, h, w, k, s, p = DGRAD[name]
    assert _wg(tile, _dgrad_rows(name, tile), COUT) >= MIN_WG
    e = _dgrad_ref(name, dtype)
    dx = _nan((n, h, w, COUT), dtype)
    T.conv2d_dgrad(e["dyv"], e["wT"], dx, kh=k, kw=k, stride=s, pad=p, dil=1, residual=e["prevv"], tile=tile)
    _check_grad(dx, e["dx"] + e["prev_nhwc"], dtype, f"{name}.dgrad/tile{tile}")


# ---------------------------------------------------------------------------------------------------------------------------
# e. fused BatchNorm backward across trips (the coefficients parked in LDS are re-read per tile)
# ---------------------------------------------------------------------------------------------------------------------------
def _row_pixels(name, tile, n):
    """dx pixel of every logical row of a data-gradient launch, -1 for none (the tail of the last tile; parity-ordered launches:
    the padding rows of a class, igemm_params.h par_out_pixel)."""
    _, h, w, k, s, p = DGRAD[name]
    bp = KTILES[tile][1]
    if s == 1:
        r = torch.arange(_cdiv(n * h * w, bp) * bp)
        return torch.where(r < n * h * w, r, -1)
    hq, wq = _cdiv(h, 2), _cdiv(w, 2)
    mq = _cdiv(n * hq * wq, bp) * bp
    r = torch.arange(4 * mq)
    q, m = r // mq, r % mq
    i, j = (m % (hq * wq)) // wq, m % wq
    hh, ww = 2 * i + q // 2, 2 * j + q % 2
    ok = (m < n * hq * wq) & (hh < h) & (ww < w)
    return torch.where(ok, ((m // (hq * wq)) * h + hh) * w + ww, -1)


def _bnb_inputs(name, with_out, dtype):
    def make():
        n = BNB_N
        _, h, w, k, s, p = DGRAD[name]
        z = _q(_rand(n, COUT, h, w, seed=131) * 0.8 + 0.3, dtype)
        gam, bet = _rand(COUT, seed=132) * 0.3 + 1.0, _rand(COUT, seed=133) * 0.3
        mean = z.mean((0, 2, 3))
        rstd = (z.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
        scale, shift = gam * rstd, bet - mean * gam * rstd
        zn = z.permute(0, 2, 3, 1).contiguous()
        e = dict(zv=_nhwc(z, dtype), zn=zn, gam=gam, mean=mean, rstd=rstd)
        e.update((k_, t.float().to(DEV)) for k_, t in (("mean_d", mean), ("rstd_d", rstd), ("sc_d", scale), ("sh_d", shift)))
        if with_out:
            skip = _q(_rand(n, COUT, h, w, seed=134), dtype)
            a = _q(F.relu(F.batch_norm(z, None, None, gam, bet, True, 0.1, 1e-5) + skip), dtype)
            e["outv"] = _nhwc(a, dtype)
            e["mask"] = (a.permute(0, 2, 3, 1) > 0).float()
        else:
            e["outv"] = None
            e["mask"] = ((zn * scale.float() + shift.float()) > 0).float()
        return e
    return _cached(("bnb", name, with_out, dtype), make, keep=1)


BNB_PARAMS = [pytest.param(name, wo, dt, t, id=f"{name}-{'out' if wo else 'z'}-{'f32' if dt == torch.float32 else 'bf16'}-tile{t}")
              for name, wo in BNB_CASES for dt in DTYPES for t in BNB_TILES]


@gpu
@pytest.mark.parametrize("name,with_out,dtype,tile", BNB_PARAMS)
def test_dgrad_fused_bn_backward_across_trips(name, with_out, dtype, tile):
    """the checks of test_gpu_train_ops.test_conv_dgrad_fused_bn_backward_stats, against the float64 data gradient: the masked
    gradient g, the sums of g and g * zhat (per pixel tile and in all), and the BatchNorm input gradient made from them.
    dy and the residual are scaled by a power of two unique to (tile, dtype): the partial sums are allocated uninitialised, and a
    slot that no tile writes must not pass with the sums of an earlier launch of the same layout."""
    from cavp_amd import ops, train_ops as T
    _, h, w, k, s, p = DGRAD[name]
    n = BNB_N
    assert _wg(tile, _dgrad_rows(name, tile, n), COUT) >= MIN_WG
    d = _dgrad_ref(name, dtype)
    b = _bnb_inputs(name, with_out, dtype)
    f = 2.0 ** (BNB_TILES.index(tile) + len(BNB_TILES) * DTYPES.index(dtype))
    dyv = d["dyv"][:n] * f
    res = d["prevv"][:n] * f if with_out else None
    ref = (d["dx"][:n] + d["prev_nhwc"][:n] if with_out else d["dx"][:n]) * f
    plain = _nan((n, h, w, COUT), dtype)   # (checked against float64 by test_dgrad_forced_tile; here through dz_ref below)
    T.conv2d_dgrad(dyv, d["wT"], plain, kh=k, kw=k, stride=s, pad=p, dil=1, residual=res, tile=tile)
    g = _nan((n, h, w, COUT), dtype)
    r = T.conv2d_dgrad(dyv, d["wT"], g, kh=k, kw=k, stride=s, pad=p, dil=1, residual=res, tile=tile,
                       bnb=dict(z=b["zv"], out=b["outv"], scale=b["sc_d"], shift=b["sh_d"], mean=b["mean_d"], rstd=b["rstd_d"],
                                act=ops.ACT_RELU))
    assert r is not None, f"tile {tile} carries the fused BatchNorm-backward statistics"
    part, tiles = r
    got_g = g.float().cpu()
    assert torch.isfinite(got_g).all(), "g: non-finite output"
    g_ref = ref * b["mask"]
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    # (a pixel whose pre-activation rounds to +-0 may flip its mask between the fused multiply-add on the device and the host's two roundings)
    bad = ((got_g - g_ref).abs() > tol * max(1.0, float(g_ref.abs().max()))).float().mean()
    assert float(bad) <= 1e-4, f"{name}: {float(bad):.2e} of the masked gradient elements differ"
    sums = torch.zeros(2, COUT, device=DEV)
    sums[0].fill_(0.25)   # cavp_bn_bwd_sum_tiles ADDS
    T.bn_bwd_sum_tiles(part, tiles, sums[0], sums[1])
    gq = got_g.double()
    zhat = (b["zn"].double() - b["mean"].double()) * b["rstd"].double()
    s0 = gq.sum((0, 1, 2)) + 0.25
    s1 = (gq * zhat).sum((0, 1, 2))
    rows = n * h * w
    stol = (2e-4 if dtype == torch.float32 else 6e-3) * (rows ** 0.5) * max(1.0, float(gq.abs().max()))
    assert float((sums[0].cpu().double() - s0).abs().max()) <= stol, (name, float((sums[0].cpu().double() - s0).abs().max()), stol)
    assert float((sums[1].cpu().double() - s1).abs().max()) <= 3 * stol, (name, float((sums[1].cpu().double() - s1).abs().max()), stol)
    # per pixel tile: the pair of every tile in its own slot
    bp = KTILES[tile][1]
    pix = _row_pixels(name, tile, n)
    assert tiles == pix.numel() // bp == part.shape[0]
    idx = torch.where(pix >= 0, pix, rows)
    gt = torch.cat([gq.view(rows, COUT), gq.new_zeros(1, COUT)])[idx].view(tiles, bp, COUT)
    zt = torch.cat([zhat.reshape(rows, COUT), zhat.new_zeros(1, COUT)])[idx].view(tiles, bp, COUT)
    pt = part.cpu().double()
    assert torch.isfinite(pt).all(), "a partial-sum slot was not written"
    ttol = (2e-4 if dtype == torch.float32 else 6e-3) * (bp ** 0.5) * max(1.0, float(gq.abs().max()))
    e0 = float((pt[:, :, 0] - gt.sum(1)).abs().max())
    e1 = float((pt[:, :, 1] - (gt * zt).sum(1)).abs().max())
    assert e0 <= ttol and e1 <= 3 * ttol, (name, e0, e1, ttol)
    # end to end: dz from the fused route == dz from the separate reduce on the plain gradient
    sums_ref = torch.zeros(2, COUT, device=DEV)
    T.bn_act_bwd_reduce(plain, b["outv"], b["zv"], b["mean_d"], b["rstd_d"], ops.ACT_RELU, sums_ref[0], sums_ref[1],
                        fwd_scale=b["sc_d"], fwd_shift=b["sh_d"])
    sums[0] -= 0.25
    dz_ref, dz = _nan(plain.shape, dtype), _nan(plain.shape, dtype)
    gam = b["gam"].to(DEV)
    T.bn_act_bwd_apply(plain, b["outv"], b["zv"], b["mean_d"], b["rstd_d"], gam, sums_ref[0], sums_ref[1], ops.ACT_RELU, dz_ref,
                       fwd_scale=b["sc_d"], fwd_shift=b["sh_d"])
    T.bn_act_bwd_apply(g, None, b["zv"], b["mean_d"], b["rstd_d"], gam, sums[0], sums[1], ops.ACT_NONE, dz)
    _check_grad(dz, dz_ref.float().cpu(), dtype, f"{name}.dz fused vs separate/tile{tile}", 2e-4, 2e-2)


# ---------------------------------------------------------------------------------------------------------------------------
# f. race screen: a ring stage reused too early by the next tile's prefetch shows up as run-to-run differences
# ---------------------------------------------------------------------------------------------------------------------------
RACE = [("fwd", "3x3_ragged", torch.float32, 8), ("fwd", "1x1_k2", BF, 12), ("dgrad", "3x3_s2_odd", BF, 11),
        ("dgrad", "1x1_s2", torch.float32, 4)]


@gpu
@pytest.mark.parametrize("kind,name,dtype,tile", RACE, ids=[f"{r[0]}-{r[1]}-{'f32' if r[2] == torch.float32 else 'bf16'}-tile{r[3]}"
                                                             for r in RACE])
def test_persistent_launch_is_race_free(kind, name, dtype, tile):
    from cavp_amd import train_ops as T
    if kind == "fwd":
        e = _fwd_ref(name, dtype)
        shape = (FWD[name][0], *_fwd_rows(name)[1:], COUT)
        run = lambda out: _fwd_launch(name, dtype, tile, e, out)   # noqa: E731
        ref, check = e["ref"], _check
    else:
        e = _dgrad_ref(name, dtype)
        n, h, w, k, s, p = DGRAD[name]
        shape = (n, h, w, COUT)
        run = lambda out: T.conv2d_dgrad(e["dyv"], e["wT"], out, kh=k, kw=k, stride=s, pad=p, dil=1, tile=tile)   # noqa: E731
        ref, check = e["dx"], _check_grad
    first = _nan(shape, dtype)
    run(first)
    check(first, ref, dtype, f"{kind} {name}/tile{tile}")
    for i in range(5):
        out = _nan(shape, dtype)
        run(out)
        assert torch.equal(out, first), f"{kind} {name}/tile{tile}: repeat {i + 1} differs"
