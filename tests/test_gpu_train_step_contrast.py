"""The native training step with the reference trainers' full objective, `l_ce + w * l_ctr` (trainer_cavp_vpo_mono.py:183-189):
the two kernels that connect the contrast chain to the tape's compute-dtype NHWC fusion map (cavp_contrast_gather_nhwc,
cavp_contrast_rows_bwd_add), CAVP.train_step(contrast=...) against the autograd route and against the reference's golden step,
and capture_train_step(contrast=...) as one / two hipGraphs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cavp_amd.synth import synth_inputs
from tests._golden_util import load_case
from tests.test_gpu_train_model import _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------------------------------------------ kernels
B2, HW, N, N_MATCH, CAP = 4, 64, 37, 21, 48
WIDTHS = [(40, 48), (304, 304), (112, 112)]


def _plan(mode, seed=5):
    """37 anchors, 21 in the match half, distinct pixels per half.  mode "host": the count as integers, index arrays of 37 rows;
    "header": the device sampler's layout at capacity 48 (rows 37 .. 47 hold -1)."""
    from cavp_amd.contrast import DevicePlan, SamplePlan
    rng = np.random.default_rng(seed)
    B = B2 // 2
    flat = np.concatenate([rng.permutation(B * HW)[:N_MATCH], rng.permutation(B * HW)[:N - N_MATCH]])
    b, p = np.divmod(flat, HW)
    lab = rng.integers(0, 3, N)
    if mode == "host":
        idx = tuple(torch.from_numpy(a.astype(np.int32)).to(DEV) for a in (b, p))
        return SamplePlan(b.astype(np.int32), p.astype(np.int32), lab.astype(np.int32), N_MATCH), idx, (N + 3) // 4 * 4, b, p
    full = [np.full(CAP, -1, dtype=np.int32) for _ in range(3)]
    for dst, src in zip(full, (b, p, lab)):
        dst[:N] = src
    header = torch.tensor([N, N_MATCH, 1, N - N_MATCH, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    ib, ip, lb = (torch.from_numpy(a).to(DEV) for a in full)
    return DevicePlan(header, ib, ip, lb, CAP, None, None, None), None, CAP, b, p


def _map(C, ld, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn((B2, HW, ld), generator=g).to(dtype).to(DEV)
    return base, base[..., :C]


@pytest.mark.parametrize("mode", ["host", "header"])
@pytest.mark.parametrize("C,ld", WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gather_nhwc(dtype, C, ld, mode):
    """A and the norms against F.normalize of the same rows in float64.  The input is read exactly in either dtype and all arithmetic
    is f32 (a sum of C squares, a square root, one division per element: a few f32 roundings), so one bar, 2e-6 of the row's largest
    magnitude, serves both dtypes; rows >= n are zero; a zero input row gives a zero row (eps clamp), not NaN."""
    from cavp_amd.contrast import anchor_rows, contrast_gather_nhwc
    plan, idx, rows, b, p = _plan(mode)
    base, x = _map(C, ld, dtype, seed=C)
    r = anchor_rows(b, p, N_MATCH, B2 // 2, HW)
    base.view(B2 * HW, ld)[int(r[3])] = 0          # one anchor with an all-zero feature row
    A = torch.full((rows, C), float("nan"), dtype=torch.float32, device=DEV)
    norms = torch.full((rows,), float("nan"), dtype=torch.float32, device=DEV)
    contrast_gather_nhwc(x, plan, idx, A, norms)
    torch.cuda.synchronize()
    x64 = base.view(B2 * HW, ld)[torch.from_numpy(r).to(DEV), :C].double().cpu()
    n64 = x64.norm(dim=1).clamp_min(1e-12)
    ref = x64 / n64[:, None]
    A, norms = A.cpu().double(), norms.cpu().double()
    assert torch.isfinite(A).all() and torch.isfinite(norms).all()
    err = (A[:N] - ref).abs().amax(dim=1)
    bar = 2e-6 * ref.abs().amax(dim=1)
    print(f"gather {dtype} C={C} {mode}: max err / bar {float((err / bar.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bar).all())
    assert bool(((norms[:N] - n64).abs() <= 2e-6 * n64).all())
    assert float(A[3].abs().max()) == 0.0
    assert float(A[N:].abs().max()) == 0.0 and bool((norms[N:] == 1.0).all())


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("mode", ["host", "header"])
@pytest.mark.parametrize("C,ld", WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_rows_bwd_add(dtype, C, ld, mode, scale):
    """g_row += scale * (dA - A <A, dA>) / norm from a random g, against float64.  f32: 2e-6 of the row's largest magnitude (the
    dot product over C terms carries a few f32 roundings of sum |A dA|, which an element that cancels to nearly zero does not
    shrink with).  bf16: every element within one bf16 ulp of the reference.  Rows outside the plan and the padding channels
    C .. ld-1 keep their bits."""
    from cavp_amd.contrast import anchor_rows, contrast_rows_bwd_add
    plan, idx, rows, b, p = _plan(mode)
    base, g = _map(C, ld, dtype, seed=100 + C)
    g0 = base.clone()
    gen = torch.Generator().manual_seed(7 + C)
    A = F.normalize(torch.randn((rows, C), generator=gen), dim=1).to(DEV)
    dA = torch.randn((rows, C), generator=gen).to(DEV)
    norms = (0.5 + 1.5 * torch.rand(rows, generator=gen)).to(DEV)
    contrast_rows_bwd_add(g, plan, idx, dA, A, norms, scale)
    torch.cuda.synchronize()
    r = torch.from_numpy(anchor_rows(b, p, N_MATCH, B2 // 2, HW)).to(DEV)
    A64, d64, n64 = A[:N].double(), dA[:N].double(), norms[:N].double()
    term = (d64 - A64 * (A64 * d64).sum(1, keepdim=True)) / n64[:, None]
    ref = g0.view(B2 * HW, ld)[r, :C].double() + scale * term
    got = base.view(B2 * HW, ld)[r, :C].double()
    err = (got - ref).abs()
    if dtype == torch.float32:
        bar = (2e-6 * ref.abs().amax(dim=1, keepdim=True)).expand_as(err)
    else:
        bar = 2.0 ** -8 * ref.abs() + 1e-30
    print(f"rows add {dtype} C={C} {mode} scale={scale}: max err / bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all())
    untouched = torch.ones((B2 * HW, ld), dtype=torch.bool, device=DEV)
    untouched[r, :C] = False
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(base.view(B2 * HW, ld).view(bits)[untouched], g0.view(B2 * HW, ld).view(bits)[untouched])
    assert not torch.equal(got, g0.view(B2 * HW, ld)[r, :C].double())


def test_unsupported_width_raises():
    from cavp_amd._lib import CavpError
    from cavp_amd.contrast import contrast_gather_nhwc, contrast_rows_bwd_add
    plan, idx, rows, _, _ = _plan("host")
    _, x = _map(36, 40, torch.bfloat16, seed=1)
    A = torch.zeros((rows, 36), dtype=torch.float32, device=DEV)
    norms = torch.ones(rows, dtype=torch.float32, device=DEV)
    with pytest.raises(CavpError, match="36"):
        contrast_gather_nhwc(x, plan, idx, A, norms)
    with pytest.raises(CavpError, match="36"):
        contrast_rows_bwd_add(x, plan, idx, A, A, norms)


def test_symm_add_takes_the_scale_from_the_host_alone_or_from_a_device_scalar_too():
    """cavp_symm_add with scale_dev == NULL (the native step's call) and with a device scalar (autograd's upstream gradient)"""
    import ctypes
    from cavp_amd import _lib
    lib = _lib.load()
    d = torch.arange(16, dtype=torch.float32, device=DEV).reshape(4, 4)
    up = torch.tensor([3.0], device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for scale_dev, ref in ((None, (d + d.t()) * 0.5), (up, (d + d.t()) * 1.5)):
        g = torch.empty_like(d)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.cavp_symm_add(ptr(d), ptr(g), 4, 0.5, None if scale_dev is None else ptr(scale_dev), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(g, ref)       # small integers and halves: exact in f32


# --------------------------------------------------------------------------------------------------------------------- step
CFG = dict(C=3, B=4, hw=(64, 64), lds=[False, False, False])


def _batch():
    """model inputs, labels and shuffle labels of test_ce_plus_contrast_through_autograd_path"""
    B = CFG["B"]
    image, audio, label = synth_inputs(B, CFG["hw"], audio_batch=2 * B, num_classes=CFG["C"], seed=21)
    label[:, 8:40, 8:48] = 1
    label[:, 44:60, 4:60] = 2
    label[:, :4] = 255
    shuf = label.clone()
    shuf[2:] = 0
    return [t.to(DEV) for t in (image, audio, label, shuf)]


def _crit(device_sampler=False, seed=0, max_views=32):
    from cavp_amd.contrast import ContrastLoss
    crit = ContrastLoss(temperature=0.1, ignore_idx=255, max_views=max_views)
    return crit.use_device_sampler(4, seed=seed) if device_sampler else crit


def _compare_grads(m1, m2, norm_bar=8e-2):
    """the bars of test_native_train_step_matches_autograd_path"""
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        if p1.grad is None:
            assert p2.grad is None, k
            continue
        assert p2.grad is not None, k
        a, b = p1.grad.double().flatten(), p2.grad.double().flatten()
        if float(a.norm()) < 1e-10:
            continue
        cos = float((a @ b) / (a.norm() * b.norm()))
        assert cos >= 0.99, (k, cos)
        if norm_bar is not None:
            assert abs(float(a.norm()) - float(b.norm())) <= norm_bar * float(a.norm()), (k, float(a.norm()), float(b.norm()))


@pytest.mark.parametrize("w", [1.0, 0.5])
def test_native_step_matches_autograd_route(w):
    """m2.train_step(contrast=crit, contrast_weight=w) == m1's autograd route `(l_ce + w * l_ctr).backward()` with the same host
    sampler stream: total loss, every gradient, the BatchNorm buffers; the reported terms are unweighted."""
    B = CFG["B"]
    image, audio, label, shuf = _batch()
    m1, _ = _build(CFG)
    m2, _ = _build(CFG)
    crit = _crit()
    out, fus, _ = m1(image, audio, None, False)
    torch.manual_seed(77)
    l_ctr = crit(fus[:B], label, fus[B:], shuf)
    l_ce = F.cross_entropy(out[:B] + out[B:] * 0.0, label, ignore_index=255)
    (l_ce + w * l_ctr).backward()
    torch.manual_seed(77)
    total = m2.train_step(image, audio, label, contrast=_crit(), label_shuffle=shuf, contrast_weight=w)
    torch.cuda.synchronize()
    assert total.shape == (1,) and total.is_cuda
    n_ce, n_ctr = (float(t.item()) for t in m2._last_losses)
    ref_total = float(l_ce.item()) + w * float(l_ctr.item())
    print(f"w={w}: native total {float(total.item()):.6f} (autograd route {ref_total:.6f}); l_ctr {n_ctr:.6f} (eager {float(l_ctr.item()):.6f})")
    assert abs(float(total.item()) - ref_total) <= 2e-4
    assert abs(n_ctr - float(l_ctr.item())) <= 1e-5 * abs(float(l_ctr.item()))
    assert abs(float(total.item()) - (n_ce + w * n_ctr)) <= 1e-6 * max(1.0, abs(n_ce + w * n_ctr))
    _compare_grads(m1, m2)
    for (k, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.allclose(b1.float(), b2.float(), atol=1e-3, rtol=1e-3), k


def test_no_qualifying_class_gives_ce_only_gradients():
    """All labels 0: the host sampler finds no class, the contrast term is 0 and adds nothing to the gradients."""
    image, audio, label, shuf = _batch()
    label, shuf = torch.zeros_like(label), torch.zeros_like(shuf)
    m1, _ = _build(CFG)
    m2, _ = _build(CFG)
    l1 = m1.train_step(image, audio, label)
    l2 = m2.train_step(image, audio, label, contrast=_crit(), label_shuffle=shuf)
    torch.cuda.synchronize()
    assert float(m2._last_losses[1].item()) == 0.0
    assert abs(float(l1.item()) - float(l2.item())) <= 2e-4
    _compare_grads(m1, m2)
    for (k, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.allclose(b1.float(), b2.float(), atol=1e-3, rtol=1e-3), k


def test_contrast_arguments_are_checked():
    from cavp_amd._lib import CavpError
    image, audio, label, shuf = _batch()
    m, _ = _build(CFG)
    with pytest.raises(CavpError):
        m.train_step(image, audio, label, contrast=_crit())                                   # label_shuffle is required
    with pytest.raises(CavpError):
        m.train_step(image, audio, label, contrast=_crit(), label_shuffle=shuf[:, :32])       # shape mismatch
    with pytest.raises(CavpError):
        m.train_step(image, audio, label, contrast=_crit(), label_shuffle=shuf.float())       # dtype mismatch
    with pytest.raises(CavpError):
        m.capture_train_step(image, audio, label, contrast=_crit(), label_shuffle=shuf)       # host sampler cannot be captured


def test_clip_shaped_native_step_matches_reference_golden():
    """c5_clip_train (B = 5: the reference's own model + ContrastLoss + autograd) through the native step with the host sampler
    seeded as the generator seeded it; the bars of test_clip_shaped_ce_plus_contrast_matches_reference_golden."""
    z, cfg = load_case("c5_clip_train")
    B = cfg["B"]
    assert B == 5
    m, _ = _build(cfg)
    image, audio, _ = synth_inputs(B, cfg["hw"], audio_batch=2 * B, num_classes=cfg["C"], seed=0)
    label = torch.from_numpy(z["label"].astype(np.int64)).to(DEV)
    label_shuf = torch.from_numpy(z["label_shuffle"].astype(np.int64)).to(DEV)
    torch.manual_seed(4321)
    m.train_step(image.to(DEV), audio.to(DEV), label, contrast=_crit(max_views=512), label_shuffle=label_shuf)
    torch.cuda.synchronize()
    l_ce, l_ctr = (float(t.item()) for t in m._last_losses)
    r_ce, r_ctr = float(z["loss_ce"][0]), float(z["loss_ctr"][0])
    print(f"clip, native step: CE {l_ce:.6f} (reference {r_ce:.6f}), contrast {l_ctr:.6f} (reference {r_ctr:.6f})")
    assert abs(l_ce - r_ce) <= 1e-4 * max(1.0, abs(r_ce))
    assert abs(l_ctr - r_ctr) <= 2e-3 * max(1.0, abs(r_ctr))
    params = dict(m.named_parameters())
    keys, vals = list(z["grad_norm_keys"]), z["grad_norm_vals"]
    rels = []
    for k, v in zip(keys, vals):
        g = params[k].grad
        assert g is not None, f"no gradient for {k}"
        rels.append(abs(float(g.double().norm()) - v) / max(v, 1e-9))
    rels = np.array(rels)
    print(f"clip, native step: gradient-norm rel. error median {np.median(rels):.2e} max {rels.max():.2e} ({keys[int(rels.argmax())]})")
    assert np.median(rels) <= 5e-3 and rels.max() <= 5e-2
    for s_ in [s_ for s_ in z.files if s_.startswith("grad_sample/")]:
        k = s_[len("grad_sample/"):]
        g = params[k].grad.detach().float().cpu().contiguous().flatten()
        smp = g[:: max(1, g.numel() // 4096)][:4096].numpy()
        a, b = smp.astype(np.float64), z[s_].astype(np.float64)
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
        assert cos >= 0.99, (k, cos)


# -------------------------------------------------------------------------------------------------------------------- graph
SEED = 1234


def test_captured_step_replays_with_fresh_anchors():
    """One hipGraph with the device sampler: a replay equals the eager native step of a twin seeded alike (the bars of
    test_train_step_hipgraph_replay_matches_eager), the next replay draws with the next offset, manual_seed() restarts the
    sequence (the loss bar of test_graph_replays_stay_correct), and four replays keep every gradient finite."""
    image, audio, label, shuf = _batch()
    m1, _ = _build(CFG)
    m2, _ = _build(CFG)
    l1 = m1.train_step(image, audio, label, contrast=_crit(True, SEED), label_shuffle=shuf)
    crit = _crit(True, 0)
    replay = m2.capture_train_step(image, audio, label, contrast=crit, label_shuffle=shuf)
    assert len(m2._train_graph) == 1
    m2.load_state_dict(m1.state_dict())
    crit.manual_seed(SEED)
    l2 = float(replay().item())
    ctr2 = float(m2._last_losses[1].item())
    off2 = crit.last_plan()["seed_offset"].cpu().tolist()
    torch.cuda.synchronize()
    print(f"graph: eager {float(l1.item()):.6f} replay {l2:.6f} (contrast term {ctr2:.6f}, {int(crit.last_plan()['header'][0])} anchors)")
    assert ctr2 > 0.0
    assert abs(float(l1.item()) - l2) <= 5e-3
    _compare_grads(m1, m2, norm_bar=None)
    replay()
    off3 = crit.last_plan()["seed_offset"].cpu().tolist()
    assert off2[2:] == off3[2:] and off2[:2] != off3[:2], (off2, off3)
    crit.manual_seed(SEED)
    l4 = float(replay().item())
    assert crit.last_plan()["seed_offset"].cpu().tolist() == off2
    assert abs(l4 - l2) <= 1e-4 * max(1.0, abs(l2)), (l2, l4)
    for _ in range(4):
        replay()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in m2.parameters() if p.grad is not None)


def test_split_capture_matches_single_graph():
    """split=True: two graphs (all contrast launches in the first), same loss as the single graph for the same seed."""
    image, audio, label, shuf = _batch()
    m1, _ = _build(CFG)
    m2, _ = _build(CFG)
    c1, c2 = _crit(True, 0), _crit(True, 0)
    r1 = m1.capture_train_step(image, audio, label, split=False, contrast=c1, label_shuffle=shuf)
    r2 = m2.capture_train_step(image, audio, label, split=True, contrast=c2, label_shuffle=shuf)
    assert len(m1._train_graph) == 1 and len(m2._train_graph) == 2
    m2.load_state_dict(m1.state_dict())
    c1.manual_seed(SEED)
    c2.manual_seed(SEED)
    l1, l2 = float(r1().item()), float(r2().item())
    torch.cuda.synchronize()
    assert float(m2._last_losses[1].item()) > 0.0
    assert abs(l1 - l2) <= 1e-4 * abs(l1), (l1, l2)
    assert all(torch.isfinite(p.grad).all() for p in m2.parameters() if p.grad is not None)


def test_bf16_step_with_device_sampler():
    """The same step in bf16: finite gradients, and the contrast term within the bf16 loss bar of test_train_step_bf16_b2_loss_only
    (6 % + 0.02) of the f32 native step's value for the same seed (same labels, hence the same anchors)."""
    image, audio, label, shuf = _batch()
    m32, _ = _build(CFG)
    m16, _ = _build(CFG, torch.bfloat16)
    m32.train_step(image, audio, label, contrast=_crit(True, SEED), label_shuffle=shuf)
    m16.train_step(image, audio, label, contrast=_crit(True, SEED), label_shuffle=shuf)
    torch.cuda.synchronize()
    c32, c16 = float(m32._last_losses[1].item()), float(m16._last_losses[1].item())
    print(f"bf16 contrast term {c16:.5f} (f32 {c32:.5f})")
    assert c32 > 0.0
    assert abs(c16 - c32) <= 0.06 * abs(c32) + 0.02, (c16, c32)
    assert all(torch.isfinite(p.grad).all() for p in m16.parameters() if p.grad is not None)
