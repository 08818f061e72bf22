"""ResNet-18 audio encoder (audio_backbone="18") on the GPU: the two new kernels alone, the encoder tap by tap against the float64
restatement (tests/_audio18_ref.py), bf16 against f32, the whole model against the composed oracle, the forward-only forward_train
branch, one hipGraph of the eval forward, and the training fence.

Bounds.  f32 taps: the project's tap bound 2e-4 * max(1, max|ref|) (tests/test_gpu_model.py).  bf16 stem output: that bound plus
2^-8 * |ref| per element - one round-to-nearest of an f32 accumulator to 8 significant bits.  bf16 encoder against the f32 path: the
bounds of tests/test_gpu_bf16_parity.py (L2-relative 2e-2, max error over max|ref| 5e-2).  Whole model: the fp32 bar 1e-3 on logits and
out_fusion, 1e-4 on attn_v (test_forward_matches_oracle_f32_and_api)."""
import functools

import pytest
import torch

from cavp_amd.synth import synth_state_dict
from tests._audio18_ref import PREFIX, args18, audio18_forward, audio_input, stem_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP = 2e-4


def _tap_bound(ref):
    return TAP * max(1.0, float(ref.abs().max()))


@functools.lru_cache(maxsize=None)
def _model(in_plane, C=5, B=2):
    from cavp_amd.cavp_model import CAVP
    a = args18(C, B)
    a.local_rank = DEV            # the SoundBank lives where the features do
    m = CAVP(50, None, num_classes=C, args=a, in_plane=in_plane)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1)
    m.load_state_dict(sd, strict=True)
    m.eval().to(DEV)
    return m, sd


def _eval_model(in_plane, dtype=torch.float32):
    m, sd = _model(in_plane)
    m.eval().set_compute_dtype(dtype)
    return m, sd


@functools.lru_cache(maxsize=None)
def _encoder_ref(in_plane, N, T, Fq):
    """(audio, fea_a f64, taps f64) - computed once per shape, shared, never modified."""
    _, sd = _model(in_plane)
    audio = audio_input(N, in_plane, T, Fq, seed=11 + N + T)
    taps = {}
    return audio, audio18_forward(audio, sd, torch.float64, taps), taps


# ---- 1. stem kernel alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 37, 20), (3, 1, 9, 7), (1, 2, 1, 1), (2, 2, 300, 64)])
def test_stem_pool_kernel_vs_f64(shape):
    from cavp_amd import ops
    N, Cin, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(100 + H)
    x = torch.randn(shape, generator=g) * 0.5
    w = torch.randn((64, Cin, 7, 7), generator=g) * (2.0 / (49 * Cin)) ** 0.5
    bn = (torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1,
          torch.rand(64, generator=g) + 0.5)   # weight, bias, running_mean != 0, running_var != 1
    ref = stem_forward(x.double(), w.double(), tuple(t.double() for t in bn))          # [N, 64, Hp, Wp]
    scale = (bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)).float()
    shift = (bn[1].double() - bn[2].double() * scale.double()).float()
    hs, ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    hp, wp = (hs - 1) // 2 + 1, (ws - 1) // 2 + 1
    assert tuple(ref.shape) == (N, 64, hp, wp)
    assert float(ref.max()) > 0
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.full((N, hp, wp, 64), float("nan"), dtype=dtype, device=DEV)
        ops.audio_stem_pool(x.to(DEV), w.to(DEV), scale.to(DEV), shift.to(DEV), out)
        torch.cuda.synchronize()
        got = out.double().cpu().permute(0, 3, 1, 2)
        err = (got - ref).abs()
        bound = _tap_bound(ref) + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0)
        print(f"stem {shape} {dtype}: max err {float(err.max()):.3e} (max|ref| {float(ref.abs().max()):.3f})")
        assert bool(torch.isfinite(got).all())
        assert bool((err <= bound).all()), float((err - bound).max())


def test_stem_pool_rejects_bad_arguments():
    from cavp_amd import ops
    from cavp_amd._lib import CavpError
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)   # noqa: E731
    with pytest.raises(CavpError):
        ops.audio_stem_pool(z(1, 3, 9, 7), z(64, 3, 7, 7), z(64), z(64), z(1, 3, 2, 64))      # three input channels
    with pytest.raises(CavpError):
        ops.audio_stem_pool(z(1, 1, 9, 7), z(64, 1, 7, 7), z(64), z(64), z(1, 3, 3, 64))      # wrong pooled shape
    with pytest.raises(CavpError):
        ops.audio_stem_pool(z(1, 1, 9, 7, dt=torch.bfloat16), z(64, 1, 7, 7), z(64), z(64), z(1, 3, 2, 64))


# ---- 2. global max -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_global_maxpool_equals_amax(dtype):
    from cavp_amd import ops
    g = torch.Generator(device="cpu").manual_seed(7)
    cases = {
        "3x20x512": torch.randn((3, 4, 5, 512), generator=g),
        "2x1x512": torch.randn((2, 1, 1, 512), generator=g),
        "all negative": -torch.rand((2, 3, 3, 512), generator=g) - 0.25,              # a zero-initialised maximum would answer 0
        "odd channels": torch.randn((2, 5, 3, 70), generator=g),                      # the scalar route
    }
    for name, x in cases.items():
        xd = x.to(dtype).to(DEV)
        out = torch.full((xd.shape[0], xd.shape[3]), float("nan"), dtype=dtype, device=DEV)
        ops.global_maxpool(xd, out)
        assert torch.equal(out, xd.amax(dim=(1, 2))), name
    wide = torch.randn((3, 4, 5, 512), generator=g).to(dtype).to(DEV)
    for name, view in (("strided view", wide[..., 128:384]), ("strided, unaligned", wide[..., 3:73])):
        out = torch.empty((3, view.shape[3]), dtype=dtype, device=DEV)
        ops.global_maxpool(view, out)
        assert torch.equal(out, view.amax(dim=(1, 2))), name
    neg = ops.global_maxpool(cases["all negative"].to(dtype).to(DEV), torch.empty((2, 512), dtype=dtype, device=DEV))
    assert float(neg.max()) < 0


# ---- 3. encoder, f32, tap by tap ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_plane,N,T,Fq", [(1, 2, 37, 20), (2, 2, 37, 20), (1, 3, 9, 7), (2, 3, 9, 7), (2, 2, 300, 64)])
def test_encoder_f32_taps_vs_f64(in_plane, N, T, Fq):
    m, _ = _eval_model(in_plane)
    audio, ref, rtaps = _encoder_ref(in_plane, N, T, Fq)
    taps = {}
    with torch.no_grad():
        fea = m._audio_hip(audio.to(DEV), m.packed(), taps)
    torch.cuda.synchronize()
    assert fea.shape == (N, 304) and fea.dtype == torch.float32
    report = {}
    for k in ("stem", "layer1", "layer2", "layer3", "layer4", "pool"):
        got, want = taps["a18." + k].double().cpu(), rtaps[k]
        assert got.shape == want.shape, k
        report[k] = float((got - want).abs().max())
        assert report[k] <= _tap_bound(want), (k, report[k], _tap_bound(want))
    report["fea_a"] = float((fea.double().cpu() - ref).abs().max())
    print(f"encoder in_plane={in_plane} {N}x{T}x{Fq}:", {k: f"{v:.2e}" for k, v in report.items()})
    assert report["fea_a"] <= _tap_bound(ref)
    assert float(ref.min()) < 0 and float(fea.min()) < 0, "fc has no activation behind it: some features are negative"


def test_encoder_rejects_wrong_input():
    from cavp_amd._lib import CavpError
    m, _ = _eval_model(2)
    with torch.no_grad():
        with pytest.raises(CavpError):
            m._audio_hip(torch.zeros(2, 1, 37, 20, device=DEV), m.packed())
        with pytest.raises(CavpError):
            m._audio_hip(torch.zeros(2, 2, 37, 20, device=DEV, dtype=torch.bfloat16), m.packed())


# ---- 4. encoder, bf16 against the f32 path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("in_plane,N,T,Fq", [(1, 2, 37, 20), (2, 2, 300, 64)])
def test_encoder_bf16_tracks_f32(in_plane, N, T, Fq):
    audio = _encoder_ref(in_plane, N, T, Fq)[0].to(DEV)
    with torch.no_grad():
        m, _ = _eval_model(in_plane, torch.float32)
        f32 = m._audio_hip(audio, m.packed()).double()
        m, _ = _eval_model(in_plane, torch.bfloat16)
        got = m._audio_hip(audio, m.packed())
        assert got.dtype == torch.bfloat16
        got = got.double()
    m.set_compute_dtype(torch.float32)
    l2 = float((got - f32).norm() / f32.norm())
    mx = float((got - f32).abs().max() / f32.abs().max())
    print(f"bf16 encoder in_plane={in_plane} {N}x{T}x{Fq}: L2-rel {l2:.3e}, max-rel {mx:.3e}")
    assert l2 <= 2e-2 and mx <= 5e-2


# ---- 5. whole model ----------------------------------------------------------------------------------------------------------
def _oracle_eval(sd, image, audio, duplicate=False):
    from oracle import cavp_oracle as O
    lds = [False, False, False]
    fea_v = O.forward_feature(O.backbone_forward(image, sd, lds, False), sd, False)
    if duplicate:
        fea_v = torch.cat((fea_v, fea_v.clone()), 0)
    fea_a = audio18_forward(audio, sd, torch.float32)
    fus, pack = O.forward_fusion(fea_v, fea_a, sd)
    return O.forward_cls(fus, sd, tuple(image.shape[-2:]), False), fus, pack


def _inputs(seed, B=2, n_audio=2, in_plane=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((B, 3, 64, 96), generator=g), audio_input(n_audio, in_plane, 37, 20, seed=seed + 1)


def test_whole_model_eval_vs_composed_oracle():
    m, sd = _eval_model(2)
    image, audio = _inputs(3)
    with torch.no_grad():
        out, fus, pack = m(image.to(DEV), audio.to(DEV), eval_mode=True)
        ro, rf, rp = _oracle_eval(sd, image, audio)
        mask = m.predict(image.to(DEV), audio.to(DEV))
        lo = m.predict_lowres(image.to(DEV), audio.to(DEV))
        out2 = m.forward_inference(image.to(DEV), audio.to(DEV))[0]
    errs = (float((out.cpu() - ro).abs().max()), float((fus.cpu() - rf).abs().max()),
            float((pack["attn_v"].cpu() - rp["attn_v"]).abs().max()), float((pack["audio"].cpu() - rp["audio"]).abs().max()))
    print("whole model: logits %.2e, out_fusion %.2e, attn_v %.2e, audio %.2e" % errs)
    assert out.shape == (2, 5, 64, 96) and errs[0] <= 1e-3 and errs[1] <= 1e-3 and errs[2] <= 1e-4
    assert errs[3] <= _tap_bound(rp["audio"]) and float(pack["audio"].min()) < 0
    assert torch.equal(out, out2)
    assert mask.dtype == torch.uint8 and torch.equal(mask.long(), out.argmax(1))
    assert tuple(lo.shape) == (2, 16, 24, 5)


@pytest.mark.parametrize("seg", ["DeepLabV3Plus", "PVT"])
def test_eval_entry_points_bf16_mono(seg):
    """in_plane = 1 and bf16 through forward / predict / predict_lowres, for both visual backbones (the encoder does not depend on
    seg_model: the PVT model only has to accept it and hand its 112 features to the fusion block)."""
    from cavp_amd.cavp_model import CAVP
    if seg == "PVT":
        a = args18(5, 2, seg_model="PVT")
        a.local_rank = DEV
        m = CAVP(50, None, num_classes=5, args=a, in_plane=1)
        m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
        m.eval().to(DEV).set_compute_dtype(torch.bfloat16)
    else:
        m, _ = _eval_model(1, torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(2)
    image, audio = torch.randn((2, 3, 64, 64), generator=g).to(DEV), audio_input(2, 1, 37, 20, seed=4).to(DEV)
    with torch.no_grad():
        out, fus, pack = m(image, audio, eval_mode=True)
        mask = m.predict(image, audio)
        lo = m.predict_lowres(image, audio)
    m.set_compute_dtype(torch.float32)
    assert out.shape == (2, 5, 64, 64) and bool(torch.isfinite(out).all())
    assert pack["audio"].shape == (2, m.latent_dim, 1, 1) and float(pack["audio"].min()) < 0
    assert torch.equal(mask.long(), out.argmax(1)) and tuple(lo.shape) == (2, 16, 16, 5) and lo.dtype == torch.bfloat16


# ---- 6. forward_train, forward only (eval BatchNorm, no grad) ---------------------------------------------------------------
def test_forward_train_no_grad_2b_and_audio_func():
    from cavp_amd.cavp_model import SoundBank
    m, sd = _eval_model(2)
    B = 2
    image, audio = _inputs(5, n_audio=2 * B)
    with torch.no_grad():
        out, fus, pack = m(image.to(DEV), audio.to(DEV), None, False)            # the trainers' call: 2B clips
        ro, rf, _ = _oracle_eval(sd, image, audio, duplicate=True)
    assert out.shape == (2 * B, 5, 64, 96)
    assert float((out.cpu() - ro).abs().max()) <= 1e-3 and float((fus.cpu() - rf).abs().max()) <= 1e-3

    idx = torch.tensor([1, 0], device=DEV)
    img_label = torch.tensor([[1, 1, 0, 0, 0], [1, 0, 0, 1, 0]], device=DEV)       # column 0 = background (zeroed by update_bank)
    info = {"shuffle_idx": idx, "mod_idx_map": {0: 3}, "image_label": img_label.clone()}
    m.memory.bank_vault.zero_()
    with torch.no_grad():
        o1, _, p1 = m(image.to(DEV), audio[:B].to(DEV), info, True, audio_func=True)
        fa = m.forward_audio(audio[:B].to(DEV), {**info, "image_label": img_label.clone()}, ow_flag=False)
    a1 = p1["audio"][:, :, 0, 0]
    assert a1.shape == (2 * B, 304) and torch.equal(a1[B:], a1[:B][idx]) and torch.equal(fa, a1)
    with torch.no_grad():
        o2 = m(image.to(DEV), torch.cat((audio[:B], audio[:B][idx.cpu()])).to(DEV), None, False)[0]
    assert torch.equal(o1, o2)
    # host replay of the bank: clip 0 is the only one of class 1, clip 1 of class 3
    bank = SoundBank(out_dim=304, args=args18(5, B), device="cpu")
    bank.update_bank(a1[:B].cpu(), img_label.cpu().clone())
    assert float(bank.bank_vault.abs().max()) > 0
    assert torch.equal(m.memory.bank_vault.cpu(), bank.bank_vault)
    assert torch.equal(m.memory.bank_vault[1][-1], a1[0]) and torch.equal(m.memory.bank_vault[3][-1], a1[1])


# ---- 7. one hipGraph ---------------------------------------------------------------------------------------------------------
def test_eval_forward_in_one_graph_replays_bit_for_bit():
    from cavp_amd.train import _no_gc_during_capture
    m, _ = _eval_model(2)
    batches = [tuple(t.to(DEV) for t in _inputs(s)) for s in (21, 22)]
    with torch.no_grad():
        eager = [tuple(t.clone() for t in m(im, au, eval_mode=True)[:2]) for im, au in batches]
        image, audio = batches[0][0].clone(), batches[0][1].clone()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(image, audio, eval_mode=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out, fus, _ = m(image, audio, eval_mode=True)
    for k in (1, 0, 1):
        image.copy_(batches[k][0])
        audio.copy_(batches[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k][0]) and torch.equal(fus, eager[k][1]), k
    assert not torch.equal(eager[0][0], eager[1][0])


# ---- 8. the training fence ---------------------------------------------------------------------------------------------------
def _checksum(m):
    return [(k, float(v.double().sum()), float(v.double().abs().sum())) for k, v in m.state_dict().items()]


def test_training_is_fenced():
    from cavp_amd._lib import CavpError
    m, _ = _eval_model(2)
    image, audio = (t.to(DEV) for t in _inputs(8, n_audio=4))
    label = torch.zeros((2, 64, 96), dtype=torch.long, device=DEV)
    before = _checksum(m)
    had_arena = getattr(m, "_grad_arena", None)
    try:
        m.train()
        for call in (lambda: m.train_step(image, audio, label),
                     lambda: m.capture_train_step(image, audio, label),
                     lambda: m(image, audio, None, False),                                   # forward_train with gradients
                     lambda: m.forward_audio(audio[:2], {"shuffle_idx": [1, 0], "mod_idx_map": {}, "image_label": None}),
                     lambda: m.enable_graphed_autograd()):
            with pytest.raises(CavpError, match="training of the ResNet-18 audio encoder is not built yet; eval only"):
                call()
        with torch.no_grad():   # train-mode BatchNorm alone is fenced too
            with pytest.raises(CavpError, match="eval only"):
                m(image, audio, None, False)
        m.eval()
        with pytest.raises(CavpError, match="eval only"):   # eval-mode BatchNorm but gradients wanted
            m(image, audio, None, False)
    finally:
        m.eval()
    torch.cuda.synchronize()
    assert getattr(m, "_grad_arena", None) is had_arena is None, "the gradient arena must not be created by a fenced call"
    assert _checksum(m) == before
    assert all(p.grad is None for p in m.parameters())
