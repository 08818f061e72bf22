"""Training of the ResNet-18 audio encoder, the parts that need no GPU: the float64 restatement the GPU tests compare against
(tests/_audio18_train_ref.py) is well conditioned on the inputs they use, nn.AdaptiveMaxPool2d's tie rule is what the kernels are held
to, the opt-in switch and its fence, and the generic machinery (gradient arena, optimiser groups) holds the encoder's 62 tensors."""
import pytest
import torch
import torch.nn.functional as F

from tests import _audio18_train_ref as R
from tests._audio18_ref import args18


def _cavp(audio_backbone="18", in_plane=2):
    from cavp_amd.cavp_model import CAVP
    return CAVP(50, None, num_classes=5, args=args18(5, 2, audio_backbone=audio_backbone), in_plane=in_plane)


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", R.ENCODER_INPUTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_winners_lead_their_runners_up(shape, seed):
    """The condition the encoder-level GPU test rests on, on the float64 reference alone: every positive winner of the global max
    leads its runner-up by at least 3 x the tap bound, so an implementation within that bound picks the same winners."""
    ref = R.encoder_reference(shape, seed)
    gap, bound = R.margin_report(ref["taps"]["layer4"])
    print(f"{shape} seed {seed}: gap {gap:.3e}, tap bound {bound:.3e}")
    assert ref["taps"]["layer4"].shape[-2] * ref["taps"]["layer4"].shape[-1] >= 2, "a 1 x 1 map makes batch-statistics BatchNorm ill-conditioned"
    assert gap >= 3 * bound


@pytest.mark.parametrize("shape,seed", R.ENCODER_INPUTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_restatement_f32_tracks_f64(shape, seed):
    """Conditioning: the restatement in f32 against itself in float64, every parameter gradient by relative L2.  The GPU bar is 5e-3;
    a graph whose own f32 evaluation used up a tenth of it would make that bar a test of the inputs, so 5e-4 here."""
    r64 = R.encoder_reference(shape, seed)
    r32 = R.encoder_reference(shape, seed, True, torch.float32)
    assert torch.equal(r32["taps"]["arg"], r64["taps"]["arg"])
    assert float((r32["fea"].double() - r64["fea"]).abs().max()) <= R.TAP * max(1.0, float(r64["fea"].abs().max()))
    worst = max((float((r32["grads"][k].double() - g).norm() / g.norm()), k) for k, g in r64["grads"].items())
    print(f"{shape}: worst f32 / f64 gradient error {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 5e-4
    assert len(r64["grads"]) == 62 and all(g is not None for g in r64["grads"].values())


def test_running_statistics_of_the_restatement_follow_the_module():
    """20 BatchNorm modules, each updated once: momentum 0.1, unbiased variance, counter + 1; frozen statistics move nothing."""
    shape, seed = R.ENCODER_INPUTS[0]
    ref = R.encoder_reference(shape, seed)
    sd = R.model_state(shape[1])
    names = R.bn_names()
    assert len(names) == 20
    z = ref["taps"]["z"]
    m, v = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=True)
    assert torch.allclose(ref["buffers"]["bn1.running_mean"], 0.9 * sd[names[0] + ".running_mean"].double() + 0.1 * m, atol=1e-12)
    assert torch.allclose(ref["buffers"]["bn1.running_var"], 0.9 * sd[names[0] + ".running_var"].double() + 0.1 * v, atol=1e-12)
    for n in names:
        r = n[len(R.PREFIX) + 1:]
        assert int(ref["buffers"][r + ".num_batches_tracked"]) == int(sd[n + ".num_batches_tracked"]) + 1
    frozen = R.encoder_reference(shape, seed, False)
    for k, b in frozen["buffers"].items():
        assert torch.equal(b.to(sd[R.PREFIX + "." + k].dtype), sd[R.PREFIX + "." + k]), k
    assert not torch.equal(frozen["fea"], ref["fea"])


def test_tie_rule_first_maximum_in_scan_order():
    """nn.AdaptiveMaxPool2d sends the gradient to the FIRST maximum in (h, w) scan order - not amax's even split among ties."""
    x = torch.zeros(1, 3, 3, 4, dtype=torch.float64)
    x[0, 0, 1, 2] = x[0, 0, 2, 0] = 5.0           # tie: (1, 2) comes first
    x[0, 1] = -1.0                                # everything ties: position 0
    x[0, 2, 2, 3] = 7.0
    x.requires_grad_(True)
    y, idx = F.adaptive_max_pool2d(x, 1, return_indices=True)
    assert idx.flatten().tolist() == [1 * 4 + 2, 0, 2 * 4 + 3]
    y.sum().backward()
    want = torch.zeros_like(x)
    want[0, 0, 1, 2] = want[0, 1, 0, 0] = want[0, 2, 2, 3] = 1.0
    assert torch.equal(x.grad, want)
    x2 = x.detach().clone().requires_grad_(True)
    x2.amax(dim=(2, 3)).sum().backward()
    assert float(x2.grad[0, 0, 1, 2]) == 0.5, "amax splits: the rule the encoder must NOT follow"


# ---- the switch --------------------------------------------------------------------------------------------------------------------
def test_switch_is_off_by_default_and_restores_the_fence():
    from cavp_amd._lib import CavpError
    m = _cavp()
    image, audio = torch.zeros(2, 3, 64, 64), torch.zeros(4, 2, 37, 20)
    label = torch.zeros(2, 64, 64, dtype=torch.long)
    fenced = "training of the ResNet-18 audio encoder is not built yet; eval only"

    def calls():
        return (lambda: m.train_step(image, audio, label), lambda: m.capture_train_step(image, audio, label),
                lambda: m(image, audio, None, False),
                lambda: m.forward_audio(audio[:2], {"shuffle_idx": [1, 0], "mod_idx_map": {}, "image_label": None}),
                lambda: m.enable_graphed_autograd())
    m.train()
    for call in calls():
        with pytest.raises(CavpError, match=fenced):
            call()
    assert m.use_audio18_training() is m
    assert "_audio18_train" not in m.state_dict() and not any("audio18" in k for k in m.state_dict())
    m.enable_graphed_autograd()          # no longer fenced (nothing is captured before the first forward)
    m.enable_graphed_autograd(False)
    for call in calls()[:4]:             # past the fence: the CPU tensors are what stops these now, not the encoder
        with pytest.raises(CavpError) as e:
            call()
        assert fenced not in str(e.value)
    m.use_audio18_training(False)
    for call in calls():
        with pytest.raises(CavpError, match=fenced):
            call()
    assert all(p.grad is None for p in m.parameters())


def test_switch_on_a_vgg_model_raises():
    from cavp_amd._lib import CavpError
    m = _cavp("vgg", in_plane=1)
    with pytest.raises(CavpError, match="not the ResNet-18"):
        m.use_audio18_training()
    with pytest.raises(CavpError, match="not the ResNet-18"):
        m.use_audio18_training(False)


def test_sync_batchnorm_inside_the_encoder_stays_fenced_with_collectives_on(monkeypatch):
    from cavp_amd import train as TR
    from cavp_amd._lib import CavpError
    m = _cavp().use_audio18_training()
    rn = m.audio_backbone.backbone
    rn.layer1[0].bn1 = torch.nn.SyncBatchNorm(64)
    m.enable_graphed_autograd()                                # no process group: nothing to order, allowed
    monkeypatch.setattr(TR, "collectives_on", lambda: True)
    with pytest.raises(CavpError, match="SyncBatchNorm inside the ResNet-18 audio encoder"):
        m.enable_graphed_autograd()
    with pytest.raises(CavpError, match="SyncBatchNorm inside the ResNet-18 audio encoder"):
        m.train_step(torch.zeros(2, 3, 64, 64), torch.zeros(4, 2, 37, 20), torch.zeros(2, 64, 64, dtype=torch.long))
    assert getattr(m, "_grad_arena", None) is None


# ---- arena and optimiser -----------------------------------------------------------------------------------------------------------
def test_encoder_tensors_in_arena_and_adam_group():
    """The encoder's 62 trainable tensors have views in the flat arena, all in the early range (the backward finishes them before
    the backbone's); FusedSGDAdam's Adam group holds exactly them; cls_head and the position embeddings get no update."""
    from cavp_amd.optim import FusedSGDAdam
    m = _cavp()
    enc = list(m.audio_backbone.backbone.parameters())
    assert len(enc) == 62 and all(p.requires_grad for p in enc)
    arena = m.grad_arena("cpu")
    late = m._late_grad_ids()
    base = arena.flat.data_ptr()
    for p in enc:
        v = arena.views[id(p)]
        assert v.shape == p.shape and id(p) not in late
        assert (v.data_ptr() - base) // 4 >= arena.split
    skip = {id(p) for p in m.params_without_grad()}
    assert {id(p) for p in m.audio_backbone.cls_head.parameters()} <= skip and not ({id(p) for p in enc} & skip)
    opt = FusedSGDAdam(m, arena, 1e-3)
    ids = {id(p) for p in opt.params}
    assert {id(p) for p in enc} <= ids and not (skip & ids)
    table = bytes(opt.table.numpy().tobytes())
    from cavp_amd.optim import OptJob
    jobs = (OptJob * opt.njobs).from_buffer_copy(table)
    adam = [p for p, j in zip(opt.params, jobs) if j.kind == 1]
    assert {id(p) for p in adam} == {id(p) for p in enc}
