"""BatchNorm tile combine inside the apply pass (cavp_bn_tiles_scale_shift_act / cavp_bn_tiles_bwd_apply) against the two launches it
replaces, output for output, with torch.equal: the arithmetic and its order are the same, so there is no tolerance.  -m gpu.
(Device against device: the two-launch route these are compared with - and the fused launches themselves - are held to float64 in
test_gpu_bn_parity.py::test_tile_tables and ::test_launches_of_one_shape.)"""
import types

import pytest
import torch

from cavp_amd.synth import synth_inputs, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def _mods():
    from cavp_amd import _lib, ops, train_ops
    import cavp_amd.train as TR
    return _lib, ops, train_ops, TR


def _limit():
    from cavp_amd import train_ops as T
    return T.BN_FUSED_TILES   # the library's limit; that the two agree is what the `limit` / `limit+1` cases check


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _view(rows, C, ld, dt, seed, fill=None):
    """[rows][C] tensor, dense or the channel slice [8 : 8 + C] of a [rows][ld] buffer (a concat slice)."""
    if ld is None:
        return (_rand(rows, C, seed=seed) * 0.8 + 0.3).to(dt).to(DEV) if fill is None else torch.full((rows, C), fill, dtype=dt, device=DEV)
    buf = torch.full((rows, ld), float("nan") if fill is None else fill, dtype=dt, device=DEV)
    v = buf[:, 8:8 + C]
    if fill is None:
        v.copy_((_rand(rows, C, seed=seed) * 0.8 + 0.3).to(dt))
    return v


def _host_table(x, tiles, rpt):
    """per-tile (mean, M2) of x [rows][C] in the library's [tiles][C][2] layout, for tile heights col_tile_stats does not produce"""
    rows, C = x.shape
    xf = x.float()
    ts = torch.empty((tiles, C, 2), dtype=torch.float32, device=x.device)
    for t in range(tiles):
        blk = xf[t * rpt:min(rows, (t + 1) * rpt)]
        m = blk.mean(0)
        ts[t, :, 0] = m
        ts[t, :, 1] = ((blk - m) ** 2).sum(0)
    return ts


# tiles: lane wrap of the one-wave combine (63 / 64 / 65), the unrolled-loop boundary of the backward sum (112 / 113 / 128 / 129),
# the limit and the limit + 1 (added per test: the limit is the library's)
TILES = [1, 2, 63, 64, 65, 112, 113, 128, 129]
# (C, ld): 8; 48 written into a 304-wide buffer; 136 (no multiple of the 64-channel slice); 2048
WIDTHS = [(8, None), (48, 304), (136, None), (2048, None)]


def _fwd_cases():
    cases, i = [], 0
    for tiles in TILES + ["limit", "limit+1"]:
        for rpt in (64, 128):
            # every tile count at both tile heights on the narrow widths; residual / activation / dtype / momentum cycle through
            C, ld = WIDTHS[i % 3] if isinstance(tiles, str) or tiles > 65 else WIDTHS[(i // 2) % 3]
            cases.append((tiles, rpt, C, ld, i % 2 == 0, (ACT_NONE, ACT_RELU, ACT_LEAKY)[i % 3],
                          torch.bfloat16 if (i // 2) % 2 == 0 else torch.float32, 0.1 if i % 4 < 2 else None))
            i += 1
    for C, ld in WIDTHS:   # every width with both dtypes, with and without residual, at a lane-wrapping tile count
        for dt in (torch.bfloat16, torch.float32):
            for res in (False, True):
                cases.append((65, 64 if res else 128, C, ld, res, (ACT_RELU, ACT_LEAKY, ACT_NONE)[i % 3], dt, None if res else 0.1))
                i += 1
    return cases


def _id(c):
    tiles, rpt, C, ld, res, act, dt, mom = c
    return f"t{tiles}-r{rpt}-c{C}{'in' + str(ld) if ld else ''}-{'res' if res else 'nores'}-a{act}-{'bf16' if dt == torch.bfloat16 else 'f32'}-m{mom}"


@pytest.mark.parametrize("case", _fwd_cases(), ids=_id)
def test_forward_fused_equals_two_launches(case, monkeypatch):
    _lib, ops, T, TR = _mods()
    tiles, rpt, C, ld, with_res, act, dt, mom = case
    limit = _limit()
    over = tiles == "limit+1"
    tiles = limit if tiles == "limit" else limit + 1 if over else tiles
    rows = tiles * rpt - 5
    x = _view(rows, C, ld, dt, 1)
    res = _view(rows, C, ld, dt, 2) if with_res else None
    ts = T.col_tile_stats(x)[0] if rpt == 128 else _host_table(x, tiles, rpt)
    assert ts.shape == (tiles, C, 2)
    gamma = (torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5).to(DEV)
    beta = _rand(C, seed=4).to(DEV)
    track = mom is not None

    def run(fused):
        f = lambda: torch.full((C,), float("nan"), device=DEV)
        scale, shift, mean, rstd = f(), f(), f(), f()
        rm = (_rand(C, seed=5) * 0.1).to(DEV) if track else None
        rv = (torch.rand(C, generator=torch.Generator().manual_seed(6)) + 0.5).to(DEV) if track else None
        y = _view(rows, C, ld, dt, 0, fill=7.0)
        m = 0.1 if mom is None else mom
        if fused:
            T.scale_shift_act(x, scale, shift, y, act, residual=res, bn_tiles=(ts, tiles, rpt, gamma, beta, 1e-5, m, rm, rv, mean, rstd))
        else:
            T.bn_finalize_tiles(ts, tiles, rpt, rows, gamma, beta, 1e-5, m, rm, rv, scale, shift, mean, rstd)
            T.scale_shift_act(x, scale, shift, y, act, residual=res)
        torch.cuda.synchronize()
        return dict(y=y, scale=scale, shift=shift, mean=mean, rstd=rstd, running_mean=rm, running_var=rv)

    ref = run(False)
    fallbacks = []
    orig = T._bn_finalize_tiles
    monkeypatch.setattr(T, "_bn_finalize_tiles", lambda *a: (fallbacks.append(1), orig(*a))[1])
    got = run(True)
    # at or below the limit the one launch ran; one tile above it the library declines and the wrapper ran the two launches
    assert len(fallbacks) == (1 if over else 0)
    for k, v in ref.items():
        if v is None:
            assert got[k] is None
            continue
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(got[k], v), (k, float((got[k].float() - v.float()).abs().max()))
    if ld is not None:   # the rest of the concat buffer is untouched
        assert bool((got["y"]._base[:, :8] == 7.0).all()) and bool((got["y"]._base[:, 8 + C:] == 7.0).all())


def _bwd_cases():
    cases, i = [], 0
    for tiles in TILES + ["limit", "limit+1"]:
        for rpt in (64, 128):
            C, ld = WIDTHS[i % 3] if isinstance(tiles, str) or tiles > 65 else WIDTHS[(i // 2) % 3]
            cases.append((tiles, rpt, C, ld, torch.bfloat16 if (i // 2) % 2 == 0 else torch.float32))
            i += 1
    for C, ld in WIDTHS:
        for dt in (torch.bfloat16, torch.float32):
            cases.append((65, 64, C, ld, dt))
    return cases


@pytest.mark.parametrize("case", _bwd_cases(),
                         ids=lambda c: f"t{c[0]}-r{c[1]}-c{c[2]}{'in' + str(c[3]) if c[3] else ''}-{'bf16' if c[4] == torch.bfloat16 else 'f32'}")
def test_backward_fused_equals_two_launches(case, monkeypatch):
    _lib, ops, T, TR = _mods()
    tiles, rpt, C, ld, dt = case
    limit = _limit()
    over = tiles == "limit+1"
    tiles = limit if tiles == "limit" else limit + 1 if over else tiles
    rows = tiles * rpt - 5
    z = _view(rows, C, ld, dt, 11)
    dy = _view(rows, C, ld, dt, 12)
    zf = z.float()
    mean = zf.mean(0).contiguous()
    rstd = (zf.var(0, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma = (torch.rand(C, generator=torch.Generator().manual_seed(13)) + 0.5).to(DEV)
    # per-tile (sum g, sum g * zhat) in the [tiles][C][2] layout of the data-gradient epilogue
    g, gz = dy.float(), dy.float() * (zf - mean) * rstd
    pad = tiles * rpt - rows
    part = torch.stack([torch.cat([t, t.new_zeros(pad, C)]).view(tiles, rpt, C).sum(1) for t in (g, gz)], dim=-1).contiguous()

    def run(fused):
        sums = torch.zeros(2, C, device=DEV)
        dz = _view(rows, C, ld, dt, 0, fill=7.0)
        if fused:
            T.bn_act_bwd_apply(dy, None, z, mean, rstd, gamma, sums[0], sums[1], ACT_NONE, dz, tile_partials=(part, tiles))
        else:
            T.bn_bwd_sum_tiles(part, tiles, sums[0], sums[1])
            T.bn_act_bwd_apply(dy, None, z, mean, rstd, gamma, sums[0], sums[1], ACT_NONE, dz)
        torch.cuda.synchronize()
        return dz, sums

    dz_ref, sums_ref = run(False)
    fallbacks = []
    orig = T._bn_bwd_sum_tiles
    monkeypatch.setattr(T, "_bn_bwd_sum_tiles", lambda *a: (fallbacks.append(1), orig(*a))[1])
    dz, sums = run(True)
    assert len(fallbacks) == (1 if over else 0)
    assert torch.isfinite(dz_ref.float()).all() and torch.isfinite(sums_ref).all()
    assert torch.equal(dz, dz_ref), float((dz.float() - dz_ref.float()).abs().max())
    assert torch.equal(sums[0], sums_ref[0]) and torch.equal(sums[1], sums_ref[1])
    if ld is not None:
        assert bool((dz._base[:, :8] == 7.0).all()) and bool((dz._base[:, 8 + C:] == 7.0).all())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_tables_of_real_conv_launches(dt):
    """The tables as the model gets them: (mean, M2) out of a conv epilogue in the forward, (sum g, sum g * zhat) out of the
    data-gradient epilogue in the backward."""
    _lib, ops, T, TR = _mods()
    n, h, w, cin, cout = 4, 56, 56, 64, 64   # (backbone-shaped launches; 12544 rows stay within the tile limit)
    x = (_rand(n, h, w, cin, seed=21) + 0.7).to(dt).to(DEV)
    wt = (_rand(cout, cin, 3, 3, seed=22) * (cin * 9) ** -0.5).to(DEV)
    z = torch.empty((n, h, w, cout), dtype=dt, device=DEV)
    z, stats = ops.conv2d(x, ops.pack_weight(wt, dt), z, kh=3, kw=3, pad=1, want_tile_stats=True)
    ts, tiles, rpt = stats if stats is not None else T.col_tile_stats(z)   # (a split-K plan offers no statistics)
    assert tiles <= _limit()
    gamma, beta = (torch.rand(cout, generator=torch.Generator().manual_seed(23)) + 0.5).to(DEV), _rand(cout, seed=24).to(DEV)
    rows = n * h * w
    outs = []
    for fused in (False, True):
        f = lambda: torch.empty(cout, device=DEV)
        scale, shift, mean, rstd, rm, rv = f(), f(), f(), f(), torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
        y = torch.empty_like(z)
        if fused:
            T.scale_shift_act(z, scale, shift, y, ACT_RELU, bn_tiles=(ts, tiles, rpt, gamma, beta, 1e-5, 0.1, rm, rv, mean, rstd))
        else:
            T.bn_finalize_tiles(ts, tiles, rpt, rows, gamma, beta, 1e-5, 0.1, rm, rv, scale, shift, mean, rstd)
            T.scale_shift_act(z, scale, shift, y, ACT_RELU)
        outs.append((y, scale, shift, mean, rstd, rm, rv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    y, scale, shift, mean, rstd = outs[0][:5]
    # backward: the data gradient of a following 3x3 conv completes y.g and leaves the partial sums
    w2 = (_rand(64, cout, 3, 3, seed=25) * (cout * 9) ** -0.5).to(DEV)
    dy2 = _rand(n, h, w, 64, seed=26).to(dt).to(DEV)
    g = torch.empty_like(z)
    r = T.conv2d_dgrad(dy2, T.pack_weight_dgrad(w2, dt), g, kh=3, kw=3, stride=1, pad=1, dil=1,
                       bnb=dict(z=z, out=None, scale=scale, shift=shift, mean=mean, rstd=rstd, act=ACT_RELU))
    if r is None:   # (the planner chose a launch without the fused epilogue: per-tile sums of 128 rows made here instead)
        gf = g.float().view(-1, cout)
        gz = gf * (z.float().view(-1, cout) - mean) * rstd
        ptiles = gf.shape[0] // 128
        part = torch.stack([t.view(ptiles, 128, cout).sum(1) for t in (gf, gz)], dim=-1).contiguous()
    else:
        part, ptiles = r
    assert ptiles <= _limit()
    res = []
    for fused in (False, True):
        sums, dz = torch.zeros(2, cout, device=DEV), torch.empty_like(z)
        if fused:
            T.bn_act_bwd_apply(g, None, z, mean, rstd, gamma, sums[0], sums[1], ACT_NONE, dz, tile_partials=(part, ptiles))
        else:
            T.bn_bwd_sum_tiles(part, ptiles, sums[0], sums[1])
            T.bn_act_bwd_apply(g, None, z, mean, rstd, gamma, sums[0], sums[1], ACT_NONE, dz)
        res.append((dz, sums))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_train_step_switch_is_bit_identical():
    """One train_step of the c1p model at B = 2 with the combine inside the apply passes and with the two launches: identical loss and
    identical parameter gradients, bit for bit.  The forward's tile limit is raised to the backward's for the run, so that the
    one-launch route is in use in both directions on every small map."""
    _lib, ops, T, TR = _mods()
    from cavp_amd.cavp_model import CAVP
    C, B, hw = 3, 2, (64, 64)
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                 num_classes=C, batch_size=B, local_rank="cpu")
    image, audio, label = [t.to(DEV) for t in synth_inputs(B, hw, audio_batch=2 * B, num_classes=C, seed=10)]
    old, old_fwd = TR._BN_COMBINE_IN_APPLY, TR._BN_COMBINE_FWD_TILES
    calls = {"fwd": 0, "bwd": 0}
    o_ssa, o_apply = T.scale_shift_act, T.bn_act_bwd_apply

    def ssa(*a, **k):
        calls["fwd"] += k.get("bn_tiles") is not None
        return o_ssa(*a, **k)

    def apply(*a, **k):
        calls["bwd"] += k.get("tile_partials") is not None
        return o_apply(*a, **k)
    _lib.set_deterministic(True)
    try:
        T.scale_shift_act, T.bn_act_bwd_apply = ssa, apply
        TR._BN_COMBINE_FWD_TILES = TR._BN_COMBINE_BWD_TILES
        res = []
        for fused in (False, True):
            TR._BN_COMBINE_IN_APPLY = fused
            m = CAVP(50, None, num_classes=C, args=args)
            m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
            m.train().to(DEV).set_compute_dtype(torch.bfloat16)
            loss = m.train_step(image, audio, label, all_reduce=False)
            torch.cuda.synchronize()
            res.append((float(loss.item()), m._grad_arena.flat.clone(),
                        {k: v.clone() for k, v in m.state_dict().items() if "running_" in k}))
            if not fused:
                assert calls == {"fwd": 0, "bwd": 0}
        assert calls["fwd"] >= 40 and calls["bwd"] >= 10, calls
        assert res[0][0] == res[1][0], (res[0][0], res[1][0])
        assert torch.equal(res[0][1], res[1][1]), float((res[0][1] - res[1][1]).abs().max())
        for k, v in res[0][2].items():
            assert torch.equal(v, res[1][2][k]), k
    finally:
        T.scale_shift_act, T.bn_act_bwd_apply = o_ssa, o_apply
        _lib.set_deterministic(False)
        TR._BN_COMBINE_IN_APPLY, TR._BN_COMBINE_FWD_TILES = old, old_fwd
