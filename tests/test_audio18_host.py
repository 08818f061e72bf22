"""CPU-side checks of the ResNet-18 audio encoder (audio_backbone="18"): torchvision's key tree below audio_backbone.backbone, strict
loading, the constructor's other branches, and the float64 reference helper (tests/_audio18_ref.py) against the map sizes
computed by hand from the strides, and against itself in float32."""
import pytest
import torch

from cavp_amd.synth import synth_state_dict
from tests._audio18_ref import PREFIX, args18, audio18_forward, audio_input, expected_keys, map_sizes


def _model(in_plane, C=5):
    from cavp_amd.cavp_model import CAVP
    return CAVP(50, None, num_classes=C, args=args18(C), in_plane=in_plane)


@pytest.mark.parametrize("in_plane", [1, 2])
def test_key_tree_is_torchvisions_and_loads_strict(in_plane):
    from cavp_amd.cavp_model import ResNet18Audio
    m = _model(in_plane)
    assert isinstance(m.audio_backbone.backbone, ResNet18Audio)
    sd = m.state_dict()
    mine = {k[len(PREFIX) + 1:]: tuple(v.shape) for k, v in sd.items() if k.startswith(PREFIX + ".")}
    want = expected_keys(in_plane, m.latent_dim)
    assert len(want) == 122
    assert set(mine) == set(want), sorted(set(mine) ^ set(want))[:10]
    assert mine == want
    assert "audio_backbone.cls_head.weight" in sd and "audio_backbone.cls_head.bias" in sd
    skip = {id(p) for p in m.params_without_grad()}
    assert all(id(p) in skip for p in m.audio_backbone.cls_head.parameters())
    # a checkpoint of exactly these keys loads strictly, and a strict load notices a missing or an extra one
    new = synth_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed=3)
    m.load_state_dict(new, strict=True)
    assert torch.equal(m.audio_backbone.backbone.layer3[0].downsample[1].running_var, new[PREFIX + ".layer3.0.downsample.1.running_var"])
    short = dict(new)
    short.pop(PREFIX + ".layer2.0.downsample.0.weight")
    with pytest.raises(RuntimeError):
        m.load_state_dict(short, strict=True)


def test_initialisation_is_torchvisions():
    rn = _model(2).audio_backbone.backbone
    bn = rn.layer4[1].bn2
    assert float(bn.weight.detach().min()) == 1.0 and float(bn.bias.detach().abs().max()) == 0.0   # no zero-init residual
    w = rn.layer3[1].conv2.weight.detach()   # Kaiming-normal, fan_out = 256 * 9: std sqrt(2 / 2304) = 0.02946
    assert abs(float(w.std()) - (2.0 / (256 * 9)) ** 0.5) < 1.5e-3
    assert rn.conv1.bias is None and rn.conv1.weight.shape == (64, 2, 7, 7)


def test_other_constructor_branches_unchanged():
    from cavp_amd.cavp_model import CAVP, VGG, AudioModel
    m = CAVP(50, None, num_classes=2, args=args18(2, audio_backbone="vgg"))
    assert isinstance(m.audio_backbone.backbone, VGG) and len(m.state_dict()) == 417
    assert isinstance(AudioModel(18, None, 304).backbone.fc, torch.nn.Linear)
    for bad in ("34", "resnet18", 50, None):
        with pytest.raises(ValueError):
            AudioModel(bad, None, 304)


def test_containers_have_no_forward():
    from cavp_amd._lib import CavpError
    m = _model(1)
    with pytest.raises(CavpError):
        m.audio_backbone.backbone(torch.zeros(1, 1, 9, 7))


@pytest.mark.parametrize("T,Fq,want", [
    (300, 64, [(150, 32), (75, 16), (38, 8), (19, 4), (10, 2)]),
    (96, 64, [(48, 32), (24, 16), (12, 8), (6, 4), (3, 2)]),
    (37, 20, [(19, 10), (10, 5), (5, 3), (3, 2), (2, 1)]),
    (9, 7, [(5, 4), (3, 2), (2, 1), (1, 1), (1, 1)]),
])
def test_reference_helper_map_sizes(T, Fq, want):
    assert map_sizes(T, Fq) == want


@pytest.mark.parametrize("in_plane", [1, 2])
def test_reference_helper_f32_agrees_with_f64(in_plane):
    m = _model(in_plane)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1)
    assert float(sd[PREFIX + ".bn1.running_mean"].abs().max()) > 0 and float((sd[PREFIX + ".bn1.running_var"] - 1).abs().min()) > 0
    audio = audio_input(2, in_plane, 37, 20, seed=5)
    t64, t32 = {}, {}
    f64 = audio18_forward(audio, sd, torch.float64, t64)
    f32 = audio18_forward(audio, sd, torch.float32, t32)
    assert f64.shape == (2, m.latent_dim) and f64.dtype == torch.float64
    for k in t64:
        scale = max(1.0, float(t64[k].abs().max()))
        assert float((t32[k].double() - t64[k]).abs().max()) <= 1e-5 * scale, k
    assert float((f32.double() - f64).abs().max()) <= 1e-5 * max(1.0, float(f64.abs().max()))
    assert float(f64.min()) < 0 < float(f64.max())   # no activation behind fc
