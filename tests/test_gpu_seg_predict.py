"""ops.seg_predict / CAVP.predict / CAVP.predict_lowres / update_lowres on the MI355X: mask, probability map and confusion counts
computed from the low-resolution logits must be those of the full-resolution path (bilinear_to_nchw + argmax / seg_confusion),
bit for bit, and agree with torch on the CPU away from near-ties."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

from cavp_amd import _lib, ops
from cavp_amd import metrics as MT
from cavp_amd._lib import CavpError
from cavp_amd.synth import synth_inputs, synth_state_dict
from tests._golden_util import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 1e-4          # CPU top-2 gap below which a pixel's argmax may legitimately differ from torch's
MAX_EXCLUDED = 1e-3

# name: (N, hi, wi, Ho, Wo, C, ldx, K, align_corners, label dtype, NaN logit)
CASES = {
    "x4_c2_dense":    (2, 7, 5, 28, 20, 2, 2, 2, False, torch.int64, False),
    "x4_c2_padded":   (2, 7, 5, 28, 20, 2, 8, 24, False, torch.int64, False),
    "x4_c24_padded":  (2, 7, 5, 28, 20, 24, 32, 24, False, torch.int64, False),
    "x4_c71_padded":  (2, 7, 5, 28, 20, 71, 72, 71, False, torch.int64, False),
    "x4_c24_align":   (2, 7, 5, 28, 20, 24, 32, 30, True, torch.int64, False),
    "ragged_c24":     (2, 7, 5, 30, 23, 24, 32, 24, False, torch.int64, False),
    "ragged_c71":     (2, 7, 5, 30, 23, 71, 72, 80, False, torch.float32, False),
    "ragged_align":   (2, 7, 5, 30, 23, 2, 2, 2, True, torch.int64, False),
    "same_size":      (2, 6, 6, 6, 6, 24, 24, 24, False, torch.int64, False),
    "same_size_al":   (2, 6, 6, 6, 6, 2, 8, 3, True, torch.float32, False),
    "k150_global":    (2, 7, 5, 28, 20, 150, 152, 150, False, torch.int64, False),
    "f32_labels":     (2, 7, 5, 28, 20, 24, 32, 24, False, torch.float32, False),
    "nan_logit":      (2, 7, 5, 28, 20, 24, 32, 24, False, torch.int64, True),
    "model_head":     (4, 56, 56, 224, 224, 24, 24, 24, False, torch.int64, False),
    # 3 * 896 * 224 = 602 112 quads of 4 pixels: more than the 2048 workgroups x 256 threads of one grid pass
    "two_passes":     (3, 112, 112, 896, 896, 2, 2, 2, False, torch.int64, False),
}
_cache = {}


def _case(name, dtype):
    """Seeded inputs of a case and its full-resolution references, computed once: the product's own upsample (the exact
    reference) and torch's on the CPU."""
    key = (name, dtype)
    if key in _cache:
        return _cache[key]
    N, hi, wi, Ho, Wo, C, ldx, K, align, ldt, nan = CASES[name]
    # Near-ties are not what these cases test (the NaN case tests the tie rule), and bf16 storage makes exact ties likely: where a
    # border pixel copies one source pixel, the two largest of C bf16 values share a rounding bucket every few dozen draws.  So
    # the draw is repeated, judged by torch's CPU upsample alone, until at most 1e-4 of its pixels (a tenth of the cap the test
    # asserts; none at all below 10 000 pixels) have a top-2 gap under GAP.
    base = sorted(CASES).index(name) + (100 if dtype == torch.bfloat16 else 0)
    for attempt in range(50):
        g = torch.Generator().manual_seed(base + 1000 * attempt)
        buf = (torch.randn(N, hi, wi, ldx, generator=g) * 4).to(dtype)
        if nan:
            buf[1, 3, 2, 5] = float("nan")
        cpu = F.interpolate(buf[..., :C].float().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=align)
        top2 = torch.topk(cpu, 2, dim=1).values
        if int(((top2[:, 0] - top2[:, 1]) < GAP).sum()) <= 1e-4 * N * Ho * Wo:
            break
    else:
        raise AssertionError(f"{name}: no draw without near-ties in 50 attempts")
    labels = torch.randint(0, K, (N, Ho, Wo), generator=g)
    labels[:, :2] = 255                       # ignored
    labels[:, 2, ::3] = -1                    # negative: never counted
    labels[:, 3, ::2] = K + 3                 # valid label >= K: row K
    labels = labels.to(ldt)
    lo = buf.to(DEV)[..., :C]
    full = ops.bilinear_to_nchw(lo, torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=DEV), align)
    _cache[key] = dict(lo=lo, labels=labels.to(DEV), full=full, cpu=cpu, K=K, align=align, shape=(N, Ho, Wo), C=C)
    return _cache[key]


def _run(c, mask=True, prob=True, conf=True, channel=1):
    N, Ho, Wo = c["shape"]
    mk = torch.full((N, Ho, Wo), 255, dtype=torch.uint8, device=DEV) if mask else None
    pr = torch.full((N, Ho, Wo), -1.0, dtype=torch.float32, device=DEV) if prob else None
    M = torch.zeros((c["K"] + 1) * c["K"], dtype=torch.int64, device=DEV) if conf else None
    ops.seg_predict(c["lo"], (Ho, Wo), mask=mk, prob=pr, channel=channel, labels=c["labels"] if conf else None,
                    num_classes=c["K"] if conf else None, ignore=255, M=M, align_corners=c["align"])
    torch.cuda.synchronize()
    return mk, pr, M


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mask_and_counts_equal_full_resolution_path(name, dtype):
    """Zero differing pixels against argmax of the product's own upsample, and the counts of seg_confusion on that tensor."""
    c = _case(name, dtype)
    mk, _, M = _run(c, prob=False)
    ref = torch.argmax(c["full"], 1)
    ndiff = int((mk.long() != ref).sum())
    print(f"{name}: {ndiff} differing pixels of {ref.numel()}")
    assert ndiff == 0
    Mref = ops.seg_confusion(c["full"], c["labels"], c["K"], 255, torch.zeros_like(M))
    assert int(Mref.sum()) > 0 and int(Mref.view(c["K"] + 1, c["K"])[c["K"]].sum()) > 0
    assert torch.equal(M, Mref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if n != "two_passes"])
def test_prob_and_mask_against_torch_cpu(name, dtype):
    c = _case(name, dtype)
    channel = 1 if c["C"] == 2 else c["C"] - 2
    mk, pr, _ = _run(c, conf=False, channel=channel)
    cpu = c["cpu"]
    ref_p = torch.softmax(cpu, 1)[:, channel]
    got_p = pr.cpu()
    err = (got_p - ref_p).abs()
    both_nan = torch.isnan(got_p) & torch.isnan(ref_p)
    print(f"{name}: prob max err {float(err[~both_nan].max()):.2e}")
    assert bool(((err <= 1e-5) | both_nan).all())
    top2 = torch.topk(cpu, 2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < GAP           # False where the gap is NaN: the NaN channel must win there
    share = float(near.float().mean())
    print(f"{name}: {int(near.sum())} pixels with a CPU top-2 gap below {GAP:g}")
    assert share <= MAX_EXCLUDED
    same = mk.cpu().long() == torch.argmax(cpu, 1)
    assert bool((same | near).all())
    if name == "nan_logit":
        hit = torch.isnan(cpu).any(1)
        assert int(hit.sum()) > 0 and bool((mk.cpu().long()[hit] == 5).all())


@pytest.mark.parametrize("name", ["ragged_c24", "x4_c2_dense", "k150_global"])
def test_each_output_alone(name):
    c = _case(name, torch.float32)
    mk, pr, M = _run(c)
    assert int((mk == 255).sum()) == 0 or c["C"] > 255
    assert torch.equal(_run(c, prob=False, conf=False)[0], mk)
    assert torch.equal(_run(c, mask=False, conf=False)[1], pr)
    assert torch.equal(_run(c, mask=False, prob=False)[2], M)


def test_bad_arguments():
    c = _case("x4_c24_padded", torch.float32)
    N, Ho, Wo = c["shape"]
    lo, K = c["lo"], c["K"]
    with pytest.raises(CavpError):
        ops.seg_predict(lo, (Ho, Wo))                                    # no output requested
    lib = _lib.load()
    st = lib.cavp_seg_predict_nhwc(_lib.F32, ctypes.c_void_p(lo.data_ptr()), N, 7, 5, 24, 32, Ho, Wo, 0, None, None, 1, None, 0, 0,
                                   -1, None, None)
    assert st == _lib.ERR_BAD_ARG
    mask = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=DEV)
    M = torch.zeros((K + 1) * K, dtype=torch.int64, device=DEV)
    bad = [dict(mask=mask.int()), dict(mask=torch.empty((N, Ho, 2 * Wo), dtype=torch.uint8, device=DEV)[:, :, ::2]),
           dict(prob=torch.empty((N, Ho, Wo), dtype=torch.float64, device=DEV)),
           dict(prob=torch.empty((N, Ho, Wo), dtype=torch.float32, device=DEV), channel=24),
           dict(labels=c["labels"], num_classes=23, M=torch.zeros(24 * 23, dtype=torch.int64, device=DEV)),      # K < C
           dict(labels=c["labels"], num_classes=K, M=M[:-1]), dict(labels=c["labels"], num_classes=K, M=M.int()),
           dict(labels=c["labels"].int(), num_classes=K, M=M), dict(labels=c["labels"], num_classes=K), dict(M=M, num_classes=K),
           dict(mask=mask.cpu())]
    for kw in bad:
        with pytest.raises(CavpError):
            ops.seg_predict(lo, (Ho, Wo), **kw)
    with pytest.raises(CavpError):
        ops.seg_predict(lo.half(), (Ho, Wo), mask=mask)
    big = torch.zeros((1, 2, 2, 264), device=DEV)
    with pytest.raises(CavpError):
        ops.seg_predict(big, (8, 8), mask=torch.empty((1, 8, 8), dtype=torch.uint8, device=DEV))      # C > 256 with a u8 mask
    assert int(M.sum()) == 0


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _build(cfg, dtype, seg_model="DeepLabV3Plus"):
    from cavp_amd.cavp_model import CAVP
    args = types.SimpleNamespace(seg_model=seg_model, last_three_dilation_stride=cfg["lds"], audio_backbone="vgg",
                                 num_classes=cfg["C"], batch_size=cfg["B"], local_rank="cpu")
    if seg_model == "PVT":
        args.allow_random_pvt = True   # synthetic weights are loaded right after
    m = CAVP(50, None, num_classes=cfg["C"], args=args)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.eval().to(DEV).set_compute_dtype(dtype)
    return m


@pytest.fixture(scope="module")
def c1p():
    """The c1p_eval fixture's model (f32 compute), its inputs and its full-resolution logits."""
    z, cfg = load_case("c1p_eval")
    m = _build(cfg, torch.float32)
    image, audio, _ = synth_inputs(cfg["B"], cfg["hw"], num_classes=cfg["C"], seed=0)
    image, audio = image.to(DEV), audio.to(DEV)
    with torch.no_grad():
        out = m(image, audio, eval_mode=True)[0]
    torch.cuda.synchronize()
    return dict(z=z, cfg=cfg, m=m, image=image, audio=audio, out=out)


def test_predict_equals_forward_argmax_and_reference_f32(c1p):
    m, out = c1p["m"], c1p["out"]
    mask, prob = m.predict(c1p["image"], c1p["audio"], return_prob=True)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (c1p["cfg"]["B"],) + tuple(c1p["cfg"]["hw"]) and prob.shape == mask.shape
    assert torch.equal(m.predict(c1p["image"], c1p["audio"]), mask)
    assert int((mask.long() != out.argmax(1)).sum()) == 0
    assert float((prob - torch.softmax(out, 1)[:, 1]).abs().max()) <= 1e-5
    lo = m.predict_lowres(c1p["image"], c1p["audio"])
    assert lo.dtype == torch.float32 and lo.shape[0] == out.shape[0] and lo.shape[-1] == out.shape[1] and lo.shape[1] * 4 == out.shape[2]
    ref = torch.from_numpy(c1p["z"]["full/out_pred"])
    top2 = torch.topk(ref, 2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < 2e-3          # twice the 1e-3 logit bar of the f32 path
    print(f"c1p_eval: {int(near.sum())} of {near.numel()} pixels within 2e-3 of a tie in the reference")
    assert float(near.float().mean()) <= MAX_EXCLUDED
    ref_arg = ref.argmax(1)
    assert set(ref_arg.unique().tolist()) == {0, 1}
    assert bool(((mask.cpu().long() == ref_arg) | near).all())


def test_predict_equals_forward_argmax_bf16():
    _, cfg = load_case("c1p_eval")
    m = _build(cfg, torch.bfloat16)
    image, audio, _ = synth_inputs(cfg["B"], cfg["hw"], num_classes=cfg["C"], seed=0)
    image, audio = image.to(DEV), audio.to(DEV)
    with torch.no_grad():
        out = m(image, audio, eval_mode=True)[0]
    assert m.predict_lowres(image, audio).dtype == torch.bfloat16
    assert int((m.predict(image, audio).long() != out.argmax(1)).sum()) == 0


def test_predict_equals_forward_argmax_pvt():
    _, cfg = load_case("pvt_eval")
    m = _build(cfg, torch.float32, "PVT")
    image, audio, _ = synth_inputs(cfg["B"], cfg["hw"], num_classes=cfg["C"], seed=0)
    image, audio = image.to(DEV), audio.to(DEV)
    with torch.no_grad():
        out = m(image, audio, eval_mode=True)[0]
    mask = m.predict(image, audio)
    assert tuple(mask.shape) == (cfg["B"],) + tuple(cfg["hw"])
    assert int((mask.long() != out.argmax(1)).sum()) == 0


def test_predict_refuses_training_mode_batchnorm(c1p):
    m = c1p["m"]
    m.train()
    try:
        with pytest.raises(CavpError, match="eval"):
            m.predict(c1p["image"], c1p["audio"])
        with pytest.raises(CavpError, match="eval"):
            m.predict_lowres(c1p["image"], c1p["audio"])
    finally:
        m.eval()


def _labels(cfg, seed):
    y = torch.randint(0, 24, (cfg["B"],) + tuple(cfg["hw"]), generator=torch.Generator().manual_seed(seed))
    y[:, :8] = 255
    return y.to(DEV)


def test_update_lowres_equals_update(c1p):
    """Two batches; MIoU with the model's 2 classes, ForegroundDetect with K = 24 on the 2-class model as the trainer builds it."""
    m, cfg = c1p["m"], c1p["cfg"]
    old = (MT.MIoU(cfg["C"], 255, 0), MT.ForegroundDetect(24))
    new = (MT.MIoU(cfg["C"], 255, 0), MT.ForegroundDetect(24))
    for seed in (0, 7):
        image, audio, _ = synth_inputs(cfg["B"], cfg["hw"], num_classes=cfg["C"], seed=seed)
        image, audio, y = image.to(DEV), audio.to(DEV), _labels(cfg, seed + 20)
        with torch.no_grad():
            out = m(image, audio, eval_mode=True)[0]
        lo = m.predict_lowres(image, audio)
        for a, b in zip(old, new):
            a.update(out, y)
            b.update_lowres(lo, y, input_shape=cfg["hw"])
    for a, b in zip(old, new):
        assert int(a.counts().sum()) > 0 and torch.equal(a.counts(), b.counts())
        assert tuple(float(v) for v in a.get_metric_results()) == tuple(float(v) for v in b.get_metric_results())
    with pytest.raises(CavpError):
        new[0].update_lowres(lo, y, input_shape=(cfg["hw"][0] // 2, cfg["hw"][1]))


def test_update_lowres_captured_with_predict_lowres(c1p):
    from cavp_amd.train import _no_gc_during_capture
    m, cfg, image, audio = c1p["m"], c1p["cfg"], c1p["image"], c1p["audio"]
    y = _labels(cfg, 31)
    miou, fd = MT.MIoU(cfg["C"], 255, 0), MT.ForegroundDetect(24)

    def step():
        lo = m.predict_lowres(image, audio)
        miou.update_lowres(lo, y)
        fd.update_lowres(lo, y)

    step()
    torch.cuda.synchronize()
    once_m, once_f = miou.counts().clone(), fd.counts().clone()
    assert int(once_m.sum()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    miou.reset()
    fd.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(miou.counts(), 2 * once_m)
    assert torch.equal(fd.counts(), 2 * once_f)
