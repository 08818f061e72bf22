"""Training of the ResNet-18 audio encoder (audio_backbone="18", CAVP.use_audio18_training) on the GPU: the three new launches alone,
the encoder on the tape against the float64 restatement (tests/_audio18_train_ref.py) with batch and with frozen statistics, the
whole model against the composed oracle, the native step against the autograd route, the captured step with the optimiser in the graph,
and the switch.

Bounds.  Stem map: test_stem_pool_kernel_vs_f64's - the tap bound 2e-4 * max(1, max|ref|), plus 2^-8 |ref| per element in bf16.  Tile
statistics: tests/_bn_ref.py's derived bounds of the tile routes (stats_centred, finish) against float64 moments of the map the launch
RETURNED.  Encoder gradients: 5e-3 relative L2 per tensor (test_frozen_batchnorm_backward_vs_oracle's bar of a well-conditioned
backward); running statistics 1e-5 / 1e-4 (test_running_stats_and_second_step).  Whole model: test_train_step_b8_vs_oracle's bars;
native step against autograd: test_native_train_step_matches_autograd_path's; replays against eager steps:
test_train_step_hipgraph_replay_matches_eager's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _audio18_train_ref as R
from tests import _bn_ref as BN
from tests._audio18_ref import args18, audio_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF = torch.float32, torch.bfloat16


def _tap_bound(ref):
    return R.TAP * max(1.0, float(ref.abs().max()))


# ---- 1. the training stem launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 37, 20), (3, 1, 9, 7), (1, 2, 1, 1), (2, 2, 300, 64)], ids=lambda s: "x".join(map(str, s)))
def test_stem_train_map_and_tile_statistics(shape):
    """z against the float64 conv; mean / variance rebuilt from the tile table against float64 moments of the returned z, on the host
    (Chan in float64 over the f32 table) and through bn_finalize_tiles; the same for the two-launch route (fused=False)."""
    from cavp_amd import _lib
    from cavp_amd import train_ops as T
    N, Cin, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(100 + H)
    x = torch.randn(shape, generator=g) * 0.5
    w = torch.randn((64, Cin, 7, 7), generator=g) * (2.0 / (49 * Cin)) ** 0.5
    ref = F.conv2d(x.double(), w.double(), None, 2, 3)                                   # [N, 64, Hs, Ws]
    hs, ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(ref.shape) == (N, 64, hs, ws)
    rows = N * hs * ws
    tiles_c, rpt_c = C.c_int32(0), C.c_int32(0)
    assert _lib.load().cavp_audio_stem_train_layout(N, Cin, H, W, C.byref(tiles_c), C.byref(rpt_c)) == 1, "the one launch covers this shape"
    assert rpt_c.value % ws == 0 and tiles_c.value == -(-rows // rpt_c.value)
    gamma, beta = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    for dtype in (F32, BF):
        for fused in (True, False):
            z = torch.full((N, hs, ws, 64), float("nan"), dtype=dtype, device=DEV)
            ts, tiles, rpt = T.audio_stem_train(x.to(DEV), w.to(DEV), z, fused=fused)
            assert (tiles, rpt) == ((tiles_c.value, rpt_c.value) if fused else (-(-rows // 128), 128))
            assert tuple(ts.shape) == (tiles, 64, 2)
            f = lambda: torch.full((64,), float("nan"), device=DEV)   # noqa: E731
            scale, shift, mean, rstd = f(), f(), f(), f()
            T.bn_finalize_tiles(ts, tiles, rpt, rows, gamma, beta, BN.EPS, BN.MOM, None, None, scale, shift, mean, rstd)
            torch.cuda.synchronize()
            got = z.double().cpu()
            err = (got.permute(0, 3, 1, 2) - ref).abs()
            bound = _tap_bound(ref) + (2.0 ** -8 * ref.abs() if dtype == BF else 0.0)
            assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ts).all())
            assert bool((err <= bound).all()), float((err - bound).max())
            # float64 moments of the RETURNED map and the bounds of a route that sums centred squares in f32
            zz = got.reshape(rows, 64)
            m_ref, v_ref, b_mean, b_var = BN.stats_centred(zz)
            t64 = ts.double().cpu()
            cnt = torch.tensor([min(rpt, rows - t * rpt) for t in range(tiles)], dtype=torch.float64)[:, None]
            m_tab = (t64[..., 0] * cnt).sum(0) / rows
            v_tab = (t64[..., 1] + cnt * (t64[..., 0] - m_tab) ** 2).sum(0) / rows
            val, bnd = BN.finish(m_ref, v_ref, b_mean, b_var, gamma.cpu(), beta.cpu(), rows, None, None)
            ratios = dict(table_mean=BN.red_ratio(m_tab, m_ref, b_mean), table_var=BN.red_ratio(v_tab, v_ref, b_var),
                          mean=BN.red_ratio(mean.cpu(), val["mean"], bnd["mean"]), rstd=BN.red_ratio(rstd.cpu(), val["rstd"], bnd["rstd"]))
            print(f"stem train {shape} {'f32' if dtype == F32 else 'bf16'} {'one launch' if fused else 'two launches'}: z err "
                  f"{float(err.max()):.3e}; err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
            assert BN.within(ratios), ratios


def test_stem_train_rejects_and_declines():
    from cavp_amd import train_ops as T
    from cavp_amd._lib import CavpError
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=DEV)   # noqa: E731
    with pytest.raises(CavpError):
        T.audio_stem_train(z(1, 3, 9, 7), z(64, 3, 7, 7), z(1, 5, 4, 64))           # three input channels
    with pytest.raises(CavpError):
        T.audio_stem_train(z(1, 1, 9, 7), z(64, 1, 7, 7), z(1, 5, 5, 64))           # wrong map shape
    with pytest.raises(CavpError):
        T.audio_stem_train(z(1, 1, 9, 7, dt=BF), z(64, 1, 7, 7), z(1, 5, 4, 64))
    # 200 stem columns: past the launch's 32 strips of 6 - the wrapper runs the two launches (128-row tiles) and the result is the conv
    g = torch.Generator(device="cpu").manual_seed(3)
    x, w = torch.randn((1, 1, 3, 399), generator=g), torch.randn((64, 1, 7, 7), generator=g) * 0.2
    out = torch.full((1, 2, 200, 64), float("nan"), device=DEV)
    ts, tiles, rpt = T.audio_stem_train(x.to(DEV), w.to(DEV), out)
    assert (tiles, rpt) == (4, 128)
    ref = F.conv2d(x.double(), w.double(), None, 2, 3)
    assert float((out.double().cpu().permute(0, 3, 1, 2) - ref).abs().max()) <= _tap_bound(ref)


# ---- 2. global max with winner -----------------------------------------------------------------------------------------------
def _gmp_cases():
    g = torch.Generator(device="cpu").manual_seed(7)
    ties = torch.randn((2, 3, 4, 512), generator=g).clamp_(max=1.0)
    ties[0, 1, 2, :] = 2.0
    ties[0, 2, 0, :] = 2.0                              # exact tie: (1, 2) is first in scan order
    ties[1] = 0.0                                       # a whole image of zeros (behind a ReLU): position 0
    return {
        "3x20x512": torch.randn((3, 4, 5, 512), generator=g),
        "exact ties": ties,
        "all negative": -torch.rand((2, 3, 3, 512), generator=g) - 0.25,
        "odd channels": torch.randn((2, 5, 3, 70), generator=g),                      # the scalar route
        "HW = 1": torch.randn((2, 1, 1, 512), generator=g),
        "HW = 3 (fewer rows than waves)": torch.randn((2, 1, 3, 72), generator=g),
    }


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_global_maxpool_winner_and_backward(dtype):
    from cavp_amd import ops
    from cavp_amd import train_ops as T
    g = torch.Generator(device="cpu").manual_seed(8)
    for name, x in _gmp_cases().items():
        xq = x.to(dtype)
        n, h, w, c = xq.shape
        want, widx = F.adaptive_max_pool2d(xq.float().permute(0, 3, 1, 2), 1, return_indices=True)   # (bf16 values are exact in f32)
        want, widx = want.flatten(1), widx.flatten(1)
        xd = xq.to(DEV)
        out = torch.full((n, c), float("nan"), dtype=dtype, device=DEV)
        arg = torch.full((n, c), -1, dtype=torch.int32, device=DEV)
        ops.global_maxpool_arg(xd, out, arg)
        assert torch.equal(out.float().cpu(), want), name
        assert torch.equal(arg.cpu().long(), widx), name
        if name == "exact ties":
            assert bool((arg[0] == 1 * 4 + 2).all()) and bool((arg[1] == 0).all())
        plain = ops.global_maxpool(xd, torch.empty((n, c), dtype=dtype, device=DEV))
        assert torch.equal(plain, out), name
        dy = torch.randn((n, c), generator=g).to(dtype)
        dx = torch.full((n, h, w, c), float("nan"), dtype=dtype, device=DEV)
        T.global_maxpool_bwd(arg, dy.to(DEV), dx)
        scatter = torch.zeros((n, h * w, c))
        scatter.scatter_(1, widx[:, None, :], dy.float()[:, None, :])
        assert bool(torch.isfinite(dx).all()), name + ": every element is written"
        assert torch.equal(dx.float().cpu().reshape(n, h * w, c), scatter), name


def test_global_maxpool_arg_nan_wins_as_in_torch():
    """torch's rule `val > max || isnan(val)`: a NaN input gives NaN, and the winner is the LAST NaN in scan order"""
    from cavp_amd import ops
    g = torch.Generator(device="cpu").manual_seed(10)
    x = torch.randn((2, 3, 4, 72), generator=g)
    x[0, 0, 1, :] = float("nan")                   # position 1, then larger finite values behind it
    x[0, 2, 3, :8] = float("nan")                  # a second NaN at position 11 in the first 8 channels: the last one wins
    x[0, 0, 2, :] = 50.0
    want, widx = F.adaptive_max_pool2d(x.permute(0, 3, 1, 2), 1, return_indices=True)
    want, widx = want.flatten(1), widx.flatten(1)
    assert bool(torch.isnan(want[0]).all()) and widx[0, :8].tolist() == [11] * 8 and widx[0, 8:].tolist() == [1] * 64
    for view in (x, x[..., :70]):                  # the vector and the scalar route
        c = view.shape[3]
        out, arg = torch.zeros((2, c), device=DEV), torch.full((2, c), -1, dtype=torch.int32, device=DEV)
        ops.global_maxpool_arg(view.to(DEV), out, arg)
        assert torch.equal(torch.isnan(out).cpu(), torch.isnan(want[:, :c]))
        assert torch.equal(out[1].cpu(), want[1, :c]) and torch.equal(arg.cpu().long(), widx[:, :c])


def test_global_maxpool_arg_of_a_channel_slice():
    from cavp_amd import ops
    g = torch.Generator(device="cpu").manual_seed(9)
    wide = torch.randn((3, 4, 5, 512), generator=g).to(DEV)
    for view in (wide[..., 128:384], wide[..., 3:73]):
        n, c = 3, view.shape[3]
        out, arg = torch.empty((n, c), device=DEV), torch.empty((n, c), dtype=torch.int32, device=DEV)
        ops.global_maxpool_arg(view, out, arg)
        want, widx = F.adaptive_max_pool2d(view.permute(0, 3, 1, 2), 1, return_indices=True)
        assert torch.equal(out, want.flatten(1)) and torch.equal(arg.long(), widx.flatten(1))


# ---- 3. the encoder on the tape ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(in_plane, Cc=5, B=2):
    from cavp_amd.cavp_model import CAVP
    a = args18(Cc, B)
    a.local_rank = DEV
    m = CAVP(50, None, num_classes=Cc, args=a, in_plane=in_plane)
    m.to(DEV)
    return m


def _fresh(in_plane, Cc=5, B=2, dtype=F32, train=True):
    """the shared model with its synthetic weights and buffers put back, no gradients, training switched on"""
    m = _model(in_plane, Cc, B)
    m.load_state_dict(R.model_state(in_plane, Cc, B), strict=True)
    m.zero_grad(set_to_none=True)
    m.__dict__["_graphed_autograd"] = None
    m.train(train).set_compute_dtype(dtype)
    m.use_audio18_training()
    return m


def _encoder_on_tape(shape, seed, bn_train):
    ref = R.encoder_reference(shape, seed, bn_train)
    m = _fresh(shape[1])
    if not bn_train:
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.eval()
    info = {"shuffle_idx": ref["idx"].tolist(), "mod_idx_map": {}, "image_label": None}
    fea = m.forward_audio(ref["audio"].to(DEV), info, ow_flag=False)
    assert fea.requires_grad and fea.shape == ref["fea"].shape and fea.dtype == F32
    fea.backward(ref["dout"].to(DEV))
    torch.cuda.synchronize()
    err = float((fea.detach().double().cpu() - ref["fea"]).abs().max())
    assert err <= _tap_bound(ref["fea"]), (err, _tap_bound(ref["fea"]))
    got = dict(m.audio_backbone.backbone.named_parameters())
    worst = (0.0, None)
    for k, gref in ref["grads"].items():
        assert got[k].grad is not None, k
        e = float((got[k].grad.detach().double().cpu() - gref).norm() / gref.norm())
        worst = max(worst, (e, k))
    print(f"encoder on tape {shape} {'batch' if bn_train else 'frozen'} statistics: fea_a err {err:.2e}; worst gradient rel L2 {worst[0]:.2e} "
          f"({worst[1]})")
    assert worst[0] <= 5e-3, worst
    assert all(p.grad is None for p in m.audio_backbone.cls_head.parameters())
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("audio_backbone."))
    return m, ref


@pytest.mark.parametrize("shape,seed", R.ENCODER_INPUTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_encoder_on_tape_vs_f64(shape, seed):
    ref = R.encoder_reference(shape, seed)
    gap, bound = R.margin_report(ref["taps"]["layer4"])
    assert gap >= 3 * bound, "the test must not hang on which of two near-equal values wins the global max"
    m, ref = _encoder_on_tape(shape, seed, True)
    sd0 = R.model_state(shape[1])
    bufs = dict(m.audio_backbone.backbone.named_buffers())
    names = [n[len(R.PREFIX) + 1:] for n in R.bn_names()]
    assert len(names) == 20
    for r in names:
        assert float((bufs[r + ".running_mean"].double().cpu() - ref["buffers"][r + ".running_mean"]).abs().max()) <= 1e-5, r
        assert float((bufs[r + ".running_var"].double().cpu() - ref["buffers"][r + ".running_var"]).abs().max()) <= 1e-4, r
        assert int(bufs[r + ".num_batches_tracked"]) == int(ref["buffers"][r + ".num_batches_tracked"]) \
            == int(sd0[R.PREFIX + "." + r + ".num_batches_tracked"]) + 1, r
    # nothing outside the encoder moved
    for k, v in m.state_dict().items():
        if not k.startswith(R.PREFIX + "."):
            assert torch.equal(v.cpu(), sd0[k]), k


@pytest.mark.parametrize("shape,seed", R.ENCODER_INPUTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_encoder_on_tape_frozen_statistics(shape, seed):
    m, _ = _encoder_on_tape(shape, seed, False)
    sd0 = R.model_state(shape[1])
    for k, v in m.state_dict().items():
        if "running_" in k or "num_batches" in k:
            assert torch.equal(v.cpu(), sd0[k]), k


def test_encoder_two_launch_stem_gives_the_same(monkeypatch):
    """_FUSE_AUDIO_STEM = False (conv_smallcin_kxk + col_tile_stats): same bars."""
    from cavp_amd import train as TR
    monkeypatch.setattr(TR, "_FUSE_AUDIO_STEM", False)
    _encoder_on_tape(*R.ENCODER_INPUTS[0], True)


# ---- 4. whole model ----------------------------------------------------------------------------------------------------------
WM = dict(C=3, B=8, hw=(64, 64))


@functools.lru_cache(maxsize=None)
def _whole_inputs(seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, Cc = WM["B"], WM["C"]
    image = torch.randn((B, 3) + WM["hw"], generator=g)
    label = torch.randint(0, Cc, (B,) + WM["hw"], generator=g)
    label[torch.rand((B,) + WM["hw"], generator=g) < 0.02] = 255
    return image, audio_input(2 * B, 2, 37, 20, seed=seed + 1), label


@functools.lru_cache(maxsize=None)
def _whole_ref():
    image, audio, label = _whole_inputs()
    return R.whole_model_reference(R.model_state(2, WM["C"], WM["B"]), image, audio, label, WM["B"])


@pytest.mark.parametrize("dtype,norm_tol,cos_tol", [(F32, 5e-3, 0.9995), (BF, 0.25, None)], ids=["f32", "bf16"])
def test_whole_model_train_vs_composed_oracle(dtype, norm_tol, cos_tol):
    from cavp_amd import train_ops as T
    B = WM["B"]
    image, audio, label = _whole_inputs()
    m = _fresh(2, WM["C"], B, dtype)
    out, fus, pack = m(image.to(DEV), audio.to(DEV), None, False)
    loss, dl = T.ce_loss(out.detach(), label.to(DEV), B)
    out.backward(dl)
    torch.cuda.synchronize()
    ref_out, ref_loss, ref_g, _ = _whole_ref()
    assert abs(float(loss.item()) - ref_loss) <= (1e-4 if dtype == F32 else 6e-2) * max(1.0, abs(ref_loss)), (float(loss.item()), ref_loss)
    params = dict(m.named_parameters())
    rels, coss = [], []
    n_audio = 0
    for k, g in ref_g.items():
        mine = params[k].grad
        assert mine is not None, k
        a, b = mine.detach().double().cpu().flatten(), g.double().flatten()
        nb = float(b.norm())
        if nb < 1e-8:
            continue
        n_audio += k.startswith(R.PREFIX + ".")
        rels.append(abs(float(a.norm()) - nb) / nb)
        coss.append(float((a @ b) / (a.norm() * b.norm() + 1e-30)))
    rels, coss = np.array(rels), np.array(coss)
    print(f"{dtype}: loss {float(loss.item()):.5f} (oracle {ref_loss:.5f}); grad norm rel err median {np.median(rels):.2e} "
          f"max {rels.max():.2e}; cosine min {coss.min():.5f} median {np.median(coss):.6f}")
    assert n_audio == 62
    assert all(p.grad is None for p in m.params_without_grad())
    assert np.median(rels) <= norm_tol and rels.max() <= 12 * norm_tol
    if cos_tol is not None:
        assert np.median(coss) >= cos_tol and coss.min() >= 1 - 6 * (1 - cos_tol)


def test_native_train_step_matches_autograd_route():
    from cavp_amd import train_ops as T
    B = WM["B"]
    image, audio, label = (t.to(DEV) for t in _whole_inputs())
    m = _fresh(2, WM["C"], B)
    out, _, _ = m(image, audio, None, False)
    loss1, dl = T.ce_loss(out.detach(), label, B)
    out.backward(dl)
    g1 = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    b1 = {k: v.clone() for k, v in m.named_buffers()}
    m = _fresh(2, WM["C"], B)
    loss2 = m.train_step(image, audio, label)
    torch.cuda.synchronize()
    assert abs(float(loss1.item()) - float(loss2.item())) <= 2e-4
    assert abs(float(loss2.item()) - _whole_ref()[1]) <= 1e-4 * max(1.0, abs(_whole_ref()[1]))
    for k, p in m.named_parameters():
        if k not in g1:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        a, b = g1[k].double().flatten(), p.grad.double().flatten()
        if float(a.norm()) < 1e-10:
            continue
        cos = float((a @ b) / (a.norm() * b.norm()))
        assert cos >= 0.99 and abs(float(a.norm()) - float(b.norm())) <= 8e-2 * float(a.norm()), (k, cos)
    for k, b2 in m.named_buffers():
        assert torch.allclose(b1[k].float(), b2.float(), atol=1e-3, rtol=1e-3), k
    m._grad_arena = None


def test_forward_train_audio_func_and_graphed_autograd():
    """forward_train(audio_func=True): B clips, the second half gathered by shuffle_idx - equals the 2B-clip call on the gathered
    clips; enable_graphed_autograd: the two-graph node returns the eager node's logits and gradients."""
    from cavp_amd import train_ops as T
    B = 2
    g = torch.Generator(device="cpu").manual_seed(12)
    image = torch.randn((B, 3, 64, 64), generator=g).to(DEV)
    audio = audio_input(B, 2, 37, 20, seed=13).to(DEV)
    label = torch.randint(0, 5, (B, 64, 64), generator=g).to(DEV)
    idx = [1, 0]
    both = torch.cat((audio, audio[idx]))

    def run(m, *args, **kw):
        out, _, pack = m(image, *args, **kw)
        loss, dl = T.ce_loss(out.detach(), label, B)
        out.backward(dl)
        torch.cuda.synchronize()
        return out.detach().clone(), float(loss.item()), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    o1, l1, g1 = run(_fresh(2), both, None, False)
    info = {"shuffle_idx": idx, "mod_idx_map": {}, "image_label": torch.zeros((B, 5), dtype=torch.long, device=DEV)}
    o2, l2, g2 = run(_fresh(2), audio, info, False, audio_func=True)
    assert abs(l1 - l2) <= 2e-4 and float((o1 - o2).abs().max()) <= 1e-3 * max(1.0, float(o1.abs().max()))
    m = _fresh(2)
    m.enable_graphed_autograd()
    o3, l3, g3 = run(m, both, None, False)
    assert m.__dict__["_graphed_autograd"], "the step was captured"
    m.enable_graphed_autograd(False)
    assert abs(l1 - l3) <= 2e-4
    for k, a in g1.items():
        for other in (g2, g3):
            b = other[k]
            if float(a.norm()) < 1e-10:
                continue
            cos = float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm()))
            assert cos >= 0.99 and abs(float(a.norm()) - float(b.norm())) <= 8e-2 * float(a.norm()), (k, cos)


def test_pvt_backbone_trains_the_encoder_on_the_main_stream():
    """seg_model = "PVT" has no side stream: the encoder's stage runs in slot 0 behind the backbone (grouped weight gradients, the main
    zero pool).  One native step, mono: finite loss, all 62 gradients, counters + 1, and bn1's running mean against the float64
    moments of the stem map."""
    from cavp_amd.cavp_model import CAVP
    a = args18(5, 2, seg_model="PVT")
    a.local_rank = DEV
    sd = R.model_state(1, 5, 2, "PVT")
    m = CAVP(50, None, num_classes=5, args=a, in_plane=1)
    m.load_state_dict(sd, strict=True)
    m.train().to(DEV).use_audio18_training()
    g = torch.Generator(device="cpu").manual_seed(14)
    image = torch.randn((2, 3, 64, 64), generator=g)
    audio = audio_input(4, 1, 37, 20, seed=15)
    label = torch.randint(0, 5, (2, 64, 64), generator=g)
    loss = m.train_step(image.to(DEV), audio.to(DEV), label.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
    enc = dict(m.audio_backbone.backbone.named_parameters())
    assert len(enc) == 62
    for k, p in enc.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    assert all(p.grad is None for p in m.audio_backbone.cls_head.parameters())
    rn = m.audio_backbone.backbone
    assert all(int(mod.num_batches_tracked) == 1 for mod in rn.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    z = F.conv2d(audio.double(), sd[R.PREFIX + ".conv1.weight"].double(), None, 2, 3)
    want = 0.9 * sd[R.PREFIX + ".bn1.running_mean"].double() + 0.1 * z.mean((0, 2, 3))
    assert float((rn.bn1.running_mean.double().cpu() - want).abs().max()) <= 1e-5


# ---- 5. the captured step ----------------------------------------------------------------------------------------------------
def test_captured_step_with_optimizer_matches_eager_steps():
    """Two replays of capture_train_step(..., optimizer=opt) on two batches against two eager (train_step, opt.step()) pairs: loss and
    every gradient after each step; counters and running statistics of the encoder's 20 BatchNorm modules advance once per replay (equal
    to the eager model's at the native-step test's 1e-3 allclose)."""
    from cavp_amd.optim import FusedSGDAdam
    Cc, B = 2, 4
    consts = (1e-3, 0.9, 100, 0, 1e-8)

    def batch(seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn((B, 3, 64, 64), generator=g).to(DEV), audio_input(2 * B, 2, 37, 20, seed=seed + 1).to(DEV),
                torch.randint(0, Cc, (B, 64, 64), generator=g).to(DEV))
    batches = [batch(21), batch(31)]
    sd0 = R.model_state(2, Cc, B)

    def build():
        from cavp_amd.cavp_model import CAVP
        a = args18(Cc, B)
        a.local_rank = DEV
        m = CAVP(50, None, num_classes=Cc, args=a, in_plane=2)
        m.load_state_dict(sd0, strict=True)
        m.train().to(DEV).use_audio18_training()
        return m, FusedSGDAdam(m, m.grad_arena(DEV), consts[0], momentum=0.9, weight_decay=1e-4).use_device_schedule(*consts)
    m1, o1 = build()
    m2, o2 = build()
    image, audio, label = (t.clone() for t in batches[0])
    replay = m2.capture_train_step(image, audio, label, optimizer=o2)
    m2.load_state_dict(sd0)              # the two warm-up passes and the capture advanced the running statistics: put them back
    assert o2.iteration() == 0, "the capture itself trains nothing"
    bn = m2.audio_backbone.backbone.layer4[1].bn2
    for step, (im, au, lb) in enumerate(batches):
        l1 = float(m1.train_step(im, au, lb).item())
        g1 = {k: p.grad.detach().clone() for k, p in m1.named_parameters() if p.grad is not None}
        o1.step()
        image.copy_(im)
        audio.copy_(au)
        label.copy_(lb)
        l2 = float(replay().item())
        torch.cuda.synchronize()
        assert abs(l1 - l2) <= 5e-3, (step, l1, l2)
        assert int(bn.num_batches_tracked) == step + 1 and int(m2.audio_backbone.backbone.bn1.num_batches_tracked) == step + 1
        b1 = dict(m1.audio_backbone.backbone.named_buffers())
        for k, v2 in m2.audio_backbone.backbone.named_buffers():     # all 20 modules: statistics updated once, like the eager step's
            if k.endswith("num_batches_tracked"):
                assert int(v2) == int(b1[k]) == step + 1, (step, k)
            else:
                assert torch.allclose(b1[k].float(), v2.float(), atol=1e-3, rtol=1e-3), (step, k)
                assert not torch.equal(v2.cpu(), sd0[R.PREFIX + "." + k]), (step, k)
        for k, p2 in m2.named_parameters():
            if k not in g1:
                assert p2.grad is None, k
                continue
            a, b = g1[k].double().flatten(), p2.grad.double().flatten()
            if float(a.norm()) < 1e-10:
                continue
            cos = float((a @ b) / (a.norm() * b.norm()))
            assert cos >= 0.99, (step, k, cos)
    assert o1.iteration() == o2.iteration() == 2
    w2 = m2.audio_backbone.backbone.conv1.weight
    assert not torch.equal(w2.cpu(), sd0[R.PREFIX + ".conv1.weight"]), "the recorded update moved the encoder's weights"


# ---- 6. the switch -----------------------------------------------------------------------------------------------------------
def test_switch_off_by_default_and_restorable():
    from cavp_amd._lib import CavpError
    m = _fresh(2)
    m.use_audio18_training(False)        # a freshly built model's state
    image = torch.zeros((2, 3, 64, 64), device=DEV)
    audio = torch.zeros((4, 2, 37, 20), device=DEV)
    label = torch.zeros((2, 64, 64), dtype=torch.long, device=DEV)
    m.__dict__.pop("_grad_arena", None)
    before = [(k, float(v.double().sum())) for k, v in m.state_dict().items()]
    for call in (lambda: m.train_step(image, audio, label), lambda: m.capture_train_step(image, audio, label),
                 lambda: m(image, audio, None, False),
                 lambda: m.forward_audio(audio[:2], {"shuffle_idx": [1, 0], "mod_idx_map": {}, "image_label": None}),
                 lambda: m.enable_graphed_autograd()):
        with pytest.raises(CavpError, match="training of the ResNet-18 audio encoder is not built yet; eval only"):
            call()
    torch.cuda.synchronize()
    assert getattr(m, "_grad_arena", None) is None
    assert [(k, float(v.double().sum())) for k, v in m.state_dict().items()] == before
    m.use_audio18_training()
    loss = m.train_step(image, audio, label)
    assert bool(torch.isfinite(loss).all())
    m._grad_arena = None
    from cavp_amd.cavp_model import CAVP
    a = args18(5, 2, audio_backbone="vgg")
    with pytest.raises(CavpError, match="not the ResNet-18"):
        CAVP(50, None, num_classes=5, args=a).use_audio18_training()
