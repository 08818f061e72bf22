"""ContrastLoss with the opt-in device sampler (ContrastLoss.use_device_sampler): the numpy restatement of the sampling
specification against the reference's rules (CPU), and the MI355X path against the restatement, against the oracle's InfoNCE on the
sampled anchors, against the reference-anchored oracle where the sample is forced, and inside a captured hipGraph (gpu)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _contrast_sampler_ref as R
from tests.test_contrast import _inputs

DEV = "cuda:0"
TEMP, IGN = 0.1, 255


# ---------------------------------------------------------------------------------------------------------------- layouts
def _reduce(gt, size):
    """contrastive_aud.py:18-22."""
    return F.interpolate(gt.unsqueeze(1).float(), size=size, mode="nearest").squeeze(1).long().flatten(1).numpy()


def _layout_golden():
    """the layout of tests/test_contrast.py: 3 classes of >= 512 reduced pixels in image 0, gt_shuffle = 0 in image 1."""
    em, gt, es, gs = _inputs()
    return em, gt, es, gs, (56, 56)


def _layout_71(B=4, hw=(56, 56), C=304, seed=11):
    """71 classes with sizes falling like 1 / (1 + c): at 4 x 56 x 56 a handful have >= 512 pixels, about 40 have >= 64, the rest
    fewer; two ignored rows per image; labels given at the feature resolution."""
    g = torch.Generator().manual_seed(seed)
    w = 1.0 / (1.0 + torch.arange(71, dtype=torch.float64))
    gt = torch.multinomial(w, B * hw[0] * hw[1], replacement=True, generator=g).reshape((B,) + hw)
    gt[:, :2, :] = 255
    gs = gt.flatten()[torch.randperm(gt.numel(), generator=g)].reshape(gt.shape).clone()
    em = torch.randn((B, C) + hw, generator=g)
    es = em * 0.5 + torch.randn((B, C) + hw, generator=g)
    return em, gt, es, gs, hw


LAYOUTS = {"golden": _layout_golden, "c71": _layout_71}


def _check_rules(gm, gs, plan, max_views, max_classes):
    """contrastive_aud.py:76-141 as properties of a plan (gm / gs: reduced [B, hw] maps)."""
    HW = gm.shape[1]
    n, n_match, k, sample_num = (int(v) for v in plan["header"])
    flat_m, flat_s = gm.reshape(-1), gs.reshape(-1)
    fg = (flat_m > 0) & (flat_m != IGN)
    counts = np.bincount(flat_m[fg], minlength=256)
    eligible = [c for c in range(1, 256) if counts[c] >= max_views]
    assert k == min(len(eligible), max_classes) and plan["dropped"] == max(0, len(eligible) - max_classes)
    if not eligible:
        assert n == 0 and n_match == 0 and plan["idx_b"].shape[0] == 0
        return
    assert sample_num == min(max_views, int(fg.sum()), int((flat_m == 0).sum()))        # :118
    assert n == k * max_views + 2 * sample_num and n_match == n - sample_num
    idx = plan["idx_b"].astype(np.int64) * HW + plan["idx_p"]
    lab = plan["labels"]
    assert idx.shape[0] == n and lab.shape[0] == n and idx.min() >= 0 and idx.max() < flat_m.shape[0]
    for j, c in enumerate(eligible[:max_classes]):                                       # ascending classes, max_views distinct pixels each
        blk = slice(j * max_views, (j + 1) * max_views)
        assert np.all(flat_m[idx[blk]] == c) and np.all(lab[blk] == c) and np.unique(idx[blk]).shape[0] == max_views
    bg = slice(k * max_views, k * max_views + sample_num)
    assert np.all(flat_m[idx[bg]] == 0) and np.all(lab[bg] == 0) and np.unique(idx[bg]).shape[0] == sample_num
    sh = slice(n_match, n)
    assert np.all(fg[idx[sh]]) and np.array_equal(lab[sh], flat_s[idx[sh]]) and np.unique(idx[sh]).shape[0] == sample_num


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    z = np.zeros(1, dtype=np.uint64)
    assert [int(v[0]) for v in R.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = z + np.uint64(0xffffffff)
    assert [int(v[0]) for v in R.philox4x32_10(f, f, f, f, 0xffffffff, 0xffffffff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    c = [z + np.uint64(v) for v in (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    assert [int(v[0]) for v in R.philox4x32_10(*c, 0xa4093822, 0x299f31d0)] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("layout", ["golden", "c71"])
@pytest.mark.parametrize("max_views", [64, 512])
def test_restatement_obeys_reference_rules(layout, max_views):
    _, gt, _, gs, size = LAYOUTS[layout]()
    gm, gsd = _reduce(gt, size), _reduce(gs, size)
    plans = []
    for seed, offset in ((0, 0), (0, 1), (5, 0), (2 ** 40 + 3, 2 ** 33 + 1)):
        p = R.plan(gm, gsd, IGN, max_views, 254, seed, offset)
        _check_rules(gm, gsd, p, max_views, 254)
        assert int(p["header"][0]) > 0
        plans.append(p)
    # another offset / another seed: another plan
    for a in range(len(plans)):
        for b in range(a):
            assert not (np.array_equal(plans[a]["idx_b"], plans[b]["idx_b"]) and np.array_equal(plans[a]["idx_p"], plans[b]["idx_p"]))
    # the max_classes limit keeps the lowest classes
    p = R.plan(gm, gsd, IGN, max_views, 2, 0, 0)
    _check_rules(gm, gsd, p, max_views, 2)


def test_restatement_nothing_qualifies():
    _, gt, _, gs, size = _layout_71()
    gm, gsd = _reduce(gt, size), _reduce(gs, size)
    big = int(np.bincount(gm[(gm > 0) & (gm != IGN)]).max())
    p = R.plan(gm, gsd, IGN, big + 1, 8, 0, 0)      # one more than the largest foreground class holds
    _check_rules(gm, gsd, p, big + 1, 8)
    assert p["header"].tolist() == [0, 0, 0, 0]
    gm0 = np.zeros_like(gm)
    gm0[0, :40] = 3
    p = R.plan(gm0, gsd, IGN, 64, 8, 0, 0)
    assert p["header"].tolist() == [0, 0, 0, 0] and p["idx_b"].shape[0] == 0


# uniformity: one class of M pixels, pick Q, over REPS consecutive offsets.  Inclusion counts c_j have mean REPS*Q/M and, being
# counts of a uniform Q-subset, sum_j (c_j - mean)^2 / (REPS * (Q/M) * (1 - Q/M) * M / (M - 1)) is chi-square with M - 1 degrees of
# freedom (asymptotically).  Bound: its 1 - 1e-6 quantile by Wilson-Hilferty - derived, not tuned.
M, Q, REPS = 64, 16, 4000
Z_1E6 = 4.753424308822899          # standard normal quantile of 1 - 1e-6


def _chi2_bound(df):
    return df * (1.0 - 2.0 / (9.0 * df) + Z_1E6 * math.sqrt(2.0 / (9.0 * df))) ** 3


def _chi2_stat(counts):
    p = Q / M
    return float(((counts - REPS * p) ** 2).sum() / (REPS * p * (1 - p) * M / (M - 1)))


def test_reference_randperm_stays_inside_the_uniformity_bound():
    """the yardstick itself: torch.randperm(M)[:Q], the reference's selection, under the same statistic and bound."""
    g = torch.Generator().manual_seed(2024)
    counts = np.zeros(M)
    for _ in range(REPS):
        counts[torch.randperm(M, generator=g)[:Q].numpy()] += 1
    assert _chi2_stat(counts) <= _chi2_bound(M - 1)


@pytest.mark.parametrize("seed", [0, 77])
def test_restatement_pick_is_uniform(seed):
    members = np.arange(100, 100 + M, dtype=np.int64)
    counts = np.zeros(M)
    first = np.zeros(M)
    for off in range(REPS):
        sel = R.pick(0, members, Q, seed, off)
        counts[sel - 100] += 1
        first[sel[0] - 100] += 1
    assert _chi2_stat(counts) <= _chi2_bound(M - 1)
    # the ORDER is uniform too: the first row is a uniform member (plain multinomial chi-square, M - 1 degrees of freedom)
    assert float(((first - REPS / M) ** 2).sum() / (REPS / M)) <= _chi2_bound(M - 1)


# -------------------------------------------------------------------------------------------------------------------- GPU
def _crit(max_views, max_classes, seed=0):
    from cavp_amd.contrast import ContrastLoss
    crit = ContrastLoss(temperature=TEMP, ignore_idx=IGN, max_views=max_views)
    crit.use_device_sampler(max_classes, seed=seed)
    return crit


def _advance(crit, k):
    """move the device call counter to k (the sampler increments it once per forward call)."""
    crit._dev[1][1:2].fill_(k)


def _download(crit):
    p = crit.last_plan()
    h = p["header"].cpu().numpy()
    n = int(h[0])
    return {"header": h, "idx_b": p["idx_b"].cpu().numpy()[:n], "idx_p": p["idx_p"].cpu().numpy()[:n],
            "labels": p["labels"].cpu().numpy()[:n], "dropped": int(p["dropped_classes"].item()),
            "tail": p["labels"].cpu().numpy()[n:]}


def _assert_plan_equal(got, ref):
    assert got["header"].tolist() == ref["header"].tolist(), (got["header"], ref["header"])
    for k in ("idx_b", "idx_p", "labels"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.all(got["tail"] == -1)


def _to_dev(t, layout="nchw", grad=False):
    if layout == "nhwc_view":
        t = t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    else:
        t = t.to(DEV)
    return t.requires_grad_(True) if grad else t


def _cpu_reference(em, es, plan):
    """oracle.contrast_oracle.info_nce on the downloaded anchors, features normalised as contrast_oracle.contrast_loss does."""
    from oracle.contrast_oracle import info_nce
    em, es = em.detach().clone().requires_grad_(True), es.detach().clone().requires_grad_(True)
    n, n_match = int(plan["header"][0]), int(plan["header"][1])
    nm = F.normalize(em, p=2, dim=1).flatten(2).permute(0, 2, 1)
    ns = F.normalize(es, p=2, dim=1).flatten(2).permute(0, 2, 1)
    b, p = torch.from_numpy(plan["idx_b"].astype(np.int64)), torch.from_numpy(plan["idx_p"].astype(np.int64))
    anchors = torch.cat([nm[b[:n_match], p[:n_match]], ns[b[n_match:n], p[n_match:n]]], 0)
    loss = info_nce(anchors, torch.from_numpy(plan["labels"].astype(np.int64)), TEMP)
    loss.backward()
    return float(loss.item()), em.grad, es.grad


def _assert_loss_and_grads(loss, gm, gs, ref_loss, ref_gm, ref_gs):
    got = float(loss.item())
    print(f"loss {got:.8f} ref {ref_loss:.8f}")
    assert loss.dim() == 0
    assert abs(got - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (got, ref_loss)
    for name, g, r in (("d_match", gm, ref_gm), ("d_shuffle", gs, ref_gs)):
        g = g.detach().cpu()
        err, top = float((g - r).abs().max()), float(r.abs().max())
        print(f"{name}: max err {err:.3e} max|ref| {top:.3e}")
        assert err <= 2e-4 * top + 1e-10, (name, err, top)
        assert int((g.abs().sum(1) > 0).sum()) == int((r.abs().sum(1) > 0).sum()), name


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["golden", "c71"])
@pytest.mark.parametrize("max_views", [64, 512])
def test_gpu_plan_equals_restatement(layout, max_views):
    em, gt, es, gs, size = LAYOUTS[layout]()
    gm, gsd = _reduce(gt, size), _reduce(gs, size)
    max_classes = 48 if max_views == 64 else 6
    emd, esd, gtd, gsd_d = _to_dev(em), _to_dev(es), gt.to(DEV), gs.to(DEV)
    for seed, offset in ((0, 0), (0, 1), (123456789, 7), (-5, 2 ** 33 + 1), (2 ** 40 + 3, 0)):
        crit = _crit(max_views, max_classes, seed)
        _advance(crit, offset)
        crit(emd, gtd, esd, gsd_d)
        ref = R.plan(gm, gsd, IGN, max_views, max_classes, seed, offset)
        assert int(ref["header"][0]) > 0
        got = _download(crit)
        _assert_plan_equal(got, ref)
        assert got["dropped"] == ref["dropped"]
    # the call counter advances by itself
    crit(emd, gtd, esd, gsd_d)
    _assert_plan_equal(_download(crit), R.plan(gm, gsd, IGN, max_views, max_classes, seed, offset + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 25, 27), (8, 128, 128)])
def test_gpu_plan_other_sizes(shape):
    """B*h*w not a multiple of 256; a 128 x 128 map with B = 8 (131072 pixels: groups of > 1e5 members)."""
    B, h, w = shape
    g = torch.Generator().manual_seed(B)
    gt = torch.randint(0, 4, (B, h, w), generator=g)
    gt[:, 0, :] = 255
    gs = torch.randint(0, 4, (B, h, w), generator=g)
    em = torch.randn((B, 304, h, w), generator=g)
    emd, gtd, gsd = em.to(DEV), gt.to(DEV), gs.to(DEV)
    for max_views in (64, 512):
        if max_views * 4 > B * h * w:
            continue
        crit = _crit(max_views, 3, seed=9)
        for offset in (0, 1):
            crit(emd, gtd, emd, gsd)
            ref = R.plan(gt.flatten(1).numpy(), gs.flatten(1).numpy(), IGN, max_views, 3, 9, offset)
            assert int(ref["header"][2]) == 3
            _assert_plan_equal(_download(crit), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["golden", "c71"])
@pytest.mark.parametrize("mem", ["nhwc_view", "nchw"])
def test_gpu_loss_and_gradients_for_the_sampled_plan(layout, mem):
    em, gt, es, gs, size = LAYOUTS[layout]()
    max_views, max_classes = (512, 3) if layout == "golden" else (64, 48)
    emd, esd = _to_dev(em, mem, True), _to_dev(es, mem, True)
    crit = _crit(max_views, max_classes, seed=3)
    loss = crit(emd, gt.to(DEV), esd, gs.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    plan = _download(crit)
    _assert_plan_equal(plan, R.plan(_reduce(gt, size), _reduce(gs, size), IGN, max_views, max_classes, 3, 0))
    _assert_loss_and_grads(loss, emd.grad, esd.grad, *_cpu_reference(em, es, plan))


# ---- the chain's strided-f32 kernels on a hand-built plan, with the anchor count from the host (SamplePlan) and from a plan header
# (DevicePlan at capacity OP_CAP).  C = 40: less than one wave and no multiple of 64; 304: the product width.
OP_B, OP_HW, OP_N, OP_N_MATCH, OP_CAP = 2, (5, 7), 37, 21, 48
OP_CASES = [(mode, mem, C, n, n_match)
            for mode in ("host", "header") for mem in ("nchw", "nhwc_view") for C in (40, 304)
            for n, n_match in ((OP_N, OP_N_MATCH), (OP_N, 0), (OP_N, OP_N), (0, 0))     # (one half empty) x 2; an empty plan
            if n or mode == "header"]                                                  # (only a header can say n = 0)


@functools.lru_cache(maxsize=None)
def _op_inputs(C):
    g = torch.Generator().manual_seed(100 + C)
    em = torch.randn((OP_B, C) + OP_HW, generator=g)
    return em, em * 0.5 + torch.randn((OP_B, C) + OP_HW, generator=g)


@functools.lru_cache(maxsize=None)
def _op_anchors(n, n_match):
    """n anchors: distinct pixels per half, labels in {0, 1, 2}; in the layout of _download()."""
    rng = np.random.default_rng(5)
    npix = OP_B * OP_HW[0] * OP_HW[1]
    idx = np.concatenate([rng.permutation(npix)[:n_match], rng.permutation(npix)[:n - n_match]])
    b, p = np.divmod(idx, OP_HW[0] * OP_HW[1])
    return {"header": np.array([n, n_match, 0, 0], dtype=np.int32), "idx_b": b.astype(np.int32), "idx_p": p.astype(np.int32),
            "labels": rng.integers(0, 3, n).astype(np.int32)}


@functools.lru_cache(maxsize=None)
def _op_reference(C, n, n_match):
    """(loss, d_match, d_shuffle) of the reference-pinned oracle on these anchors; an empty plan: loss 0, no gradient."""
    em, es = _op_inputs(C)
    if n == 0:
        return 0.0, torch.zeros_like(em), torch.zeros_like(es)
    loss, gm, gs = _cpu_reference(em, es, _op_anchors(n, n_match))
    return loss, torch.zeros_like(em) if gm is None else gm, torch.zeros_like(es) if gs is None else gs


def _op_run(mode, mem, C, n, n_match, tail=None):
    """_InfoNCEFn forward + backward on the plan; tail: what rows >= n of a DevicePlan's arrays hold (-1 or in-range garbage)."""
    from cavp_amd.contrast import DevicePlan, SamplePlan, _InfoNCEFn
    em, es = _op_inputs(C)
    a = _op_anchors(n, n_match)
    emd, esd = _to_dev(em, mem, True), _to_dev(es, mem, True)
    if mode == "host":
        plan = SamplePlan(a["idx_b"], a["idx_p"], a["labels"], n_match)
    else:
        rng = np.random.default_rng(6)
        rows = np.full((3, OP_CAP), -1, dtype=np.int32)
        if tail == "garbage":
            rows = np.stack([rng.integers(0, hi, OP_CAP) for hi in (OP_B, OP_HW[0] * OP_HW[1], 3)]).astype(np.int32)
        rows[:, :n] = a["idx_b"], a["idx_p"], a["labels"]
        header = np.array([n, n_match, 0, 0, 0, 0, 0, 0], dtype=np.int32)
        buf = torch.from_numpy(np.concatenate([header, rows.reshape(-1)])).to(DEV)
        ib, ip, lab = buf[8:].view(3, OP_CAP)
        plan = DevicePlan(buf[:8], ib, ip, lab, OP_CAP, None, None, None)
    loss = _InfoNCEFn.apply(emd, esd, plan, TEMP, 1e-12)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), emd.grad.detach(), esd.grad.detach()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,mem,C,n,n_match", OP_CASES, ids=["-".join(str(v) for v in c) for c in OP_CASES])
def test_gpu_chain_on_a_hand_built_plan(deterministic, mode, mem, C, n, n_match):
    loss, gm, gs = _op_run(mode, mem, C, n, n_match, tail="minus1")
    _assert_loss_and_grads(loss, gm, gs, *_op_reference(C, n, n_match))
    a = _op_anchors(n, n_match)
    hw = OP_HW[0] * OP_HW[1]
    for g, lo, hi in ((gm, 0, n_match), (gs, n_match, n)):          # pixels outside the plan: exactly zero
        outside = np.ones(OP_B * hw, dtype=bool)
        outside[a["idx_b"][lo:hi].astype(np.int64) * hw + a["idx_p"][lo:hi]] = False
        rest = g.cpu().permute(0, 2, 3, 1).reshape(OP_B * hw, C)[torch.from_numpy(outside)]
        assert rest.numel() > 0 and float(rest.abs().max()) == 0.0
    if n == 0:
        assert float(loss.item()) == 0.0 and float(gm.abs().max()) == 0.0 and float(gs.abs().max()) == 0.0
    if mode == "header":
        # the rows >= n of the index and label arrays are never read: in-range garbage there changes no bit
        loss2, gm2, gs2 = _op_run(mode, mem, C, n, n_match, tail="garbage")
        assert torch.equal(loss, loss2) and torch.equal(gm, gm2) and torch.equal(gs, gs2)


def _case_a():
    g = torch.Generator().manual_seed(21)
    B, C, hw = 2, 304, (56, 56)
    gt = torch.full((B,) + hw, 255, dtype=torch.long)
    perm = torch.randperm(B * hw[0] * hw[1], generator=g)
    gt.view(-1)[perm[:64]] = 1
    gt.view(-1)[perm[64:128]] = 0
    gs = torch.randint(0, 3, (B,) + hw, generator=g)
    em = torch.randn((B, C) + hw, generator=g)
    es = em * 0.5 + torch.randn((B, C) + hw, generator=g)
    return em, gt, es, gs


def _case_b():
    g = torch.Generator().manual_seed(22)
    B, C, hw = 2, 304, (56, 56)
    gt = torch.zeros((B,) + hw, dtype=torch.long)
    gt[0, 4:10, :] = 1          # 336 pixels
    gt[0, 20:24, :] = 2         # 224
    gt[1, 8:11, :] = 3          # 168
    gt[1, 30, :40] = 4          # 40 pixels: below max_views, must be skipped
    gt[:, :2, :] = 255          # two ignored rows
    gs = torch.randint(0, 5, (B,) + hw, generator=g)
    gs[(gt > 0) & (gt != 255)] = 0
    v, w = torch.randn(256, C, generator=g), torch.randn(256, C, generator=g)
    em = v[gt].permute(0, 3, 1, 2).contiguous()
    es = w[gs].permute(0, 3, 1, 2).contiguous()
    return em, gt, es, gs


@pytest.mark.gpu
def test_gpu_forced_anchor_set_matches_reference_oracle():
    """Case A: exactly max_views pixels of class 1 and of class 0, everything else ignored: the anchor SET is forced, so the
    reference-pinned oracle (any RNG state) is the yardstick; only the summation order differs."""
    from oracle.contrast_oracle import contrast_loss
    em, gt, es, gs = _case_a()
    torch.manual_seed(0)
    ref = float(contrast_loss(em, gt, es, gs, TEMP, IGN, 64).item())
    crit = _crit(64, 1, seed=5)
    loss = crit(em.to(DEV), gt.to(DEV), es.to(DEV), gs.to(DEV))
    got = float(loss.item())
    print(f"case A: device {got:.8f} oracle {ref:.8f}")
    assert crit.last_plan()["header"].tolist() == [192, 128, 1, 64]
    assert abs(got - ref) <= 2e-5 * max(1.0, abs(ref)), (got, ref)


@pytest.mark.gpu
def test_gpu_constant_class_features_match_reference_oracle():
    """Case B: features depend on the label only and gt_shuffle = 0 on the match foreground, so every sample is the same
    multiset of anchors: loss and per-class gradient sums equal the reference-pinned oracle's for any RNG."""
    from oracle.contrast_oracle import contrast_loss
    em, gt, es, gs = _case_b()
    emc, esc = em.clone().requires_grad_(True), es.clone().requires_grad_(True)
    torch.manual_seed(0)
    ref = contrast_loss(emc, gt, esc, gs, TEMP, IGN, 128)
    ref.backward()
    emd, esd = _to_dev(em, grad=True), _to_dev(es, grad=True)
    crit = _crit(128, 4, seed=1)
    loss = crit(emd, gt.to(DEV), esd, gs.to(DEV))
    loss.backward()
    got, ref_l = float(loss.item()), float(ref.item())
    print(f"case B: device {got:.8f} oracle {ref_l:.8f}")
    h = crit.last_plan()["header"].tolist()
    assert h == [5 * 128, 4 * 128, 3, 128], h
    assert sorted(set(crit.last_plan()["labels"].cpu().numpy()[:3 * 128].tolist())) == [1, 2, 3]
    assert abs(got - ref_l) <= 2e-5 * max(1.0, abs(ref_l)), (got, ref_l)
    gd = emd.grad.detach().cpu()
    sums_got = torch.stack([gd.permute(0, 2, 3, 1)[gt == c].sum(0) for c in range(5)])
    sums_ref = torch.stack([emc.grad.permute(0, 2, 3, 1)[gt == c].sum(0) for c in range(5)])
    err, top = float((sums_got - sums_ref).abs().max()), float(sums_ref.abs().max())
    print(f"case B: per-class gradient sums max err {err:.3e} max|ref| {top:.3e}")
    assert err <= 2e-4 * top + 1e-10, (err, top)
    assert float(gd.permute(0, 2, 3, 1)[gt == 4].abs().max()) == 0.0


def _graph_capture_roundtrip(bitwise):
    em, gt, es, gs, size = _layout_golden()
    max_views, max_classes, seed, warm = 512, 3, 17, 2
    gt2 = torch.roll(gt, shifts=(1, 37), dims=(0, 2)).contiguous()      # another label map for the in-place refill
    emd, esd = _to_dev(em, "nhwc_view", True), _to_dev(es, "nhwc_view", True)
    gtd, gsd = gt.to(DEV), gs.to(DEV)
    crit = _crit(max_views, max_classes, seed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            emd.grad = esd.grad = None
            crit(emd, gtd, esd, gsd).backward()
    torch.cuda.current_stream().wait_stream(side)
    emd.grad = esd.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):           # raises if the step synchronises or copies to / from the host
        loss = crit(emd, gtd, esd, gsd)
        loss.backward()
    replays = []
    for k in range(3):
        if k == 2:
            gtd.copy_(gt2.to(DEV))          # refill in place; no cache call
        graph.replay()
        torch.cuda.synchronize()
        replays.append((_download(crit), loss.detach().clone(), emd.grad.detach().clone(), esd.grad.detach().clone()))
    # the same calls made eagerly at the same (seed, offset)
    eme, ese = _to_dev(em, "nhwc_view", True), _to_dev(es, "nhwc_view", True)
    eager = _crit(max_views, max_classes, seed)
    gte = gt.to(DEV)
    for k in range(3):
        labels = gt2 if k == 2 else gt
        if k == 2:
            gte.copy_(gt2.to(DEV))
        plan, l_g, gm_g, gs_g = replays[k]
        ref = R.plan(_reduce(labels, size), _reduce(gs, size), IGN, max_views, max_classes, seed, warm + k)
        _assert_plan_equal(plan, ref)
        if k:
            assert not np.array_equal(plan["idx_p"], replays[k - 1][0]["idx_p"])
        _advance(eager, warm + k)
        eme.grad = ese.grad = None
        l_e = eager(eme, gte, ese, gsd)
        l_e.backward()
        torch.cuda.synchronize()
        _assert_plan_equal(_download(eager), ref)
        if bitwise:
            assert torch.equal(l_g, l_e.detach()) and torch.equal(gm_g, eme.grad) and torch.equal(gs_g, ese.grad), k
        else:
            _assert_loss_and_grads(l_g, gm_g, gs_g, float(l_e.item()), eme.grad.detach().cpu(), ese.grad.detach().cpu())
    _assert_loss_and_grads(replays[2][1], replays[2][2], replays[2][3], *_cpu_reference(em, es, replays[2][0]))


@pytest.mark.gpu
def test_gpu_graph_capture_bitwise(deterministic):
    _graph_capture_roundtrip(bitwise=True)


@pytest.mark.gpu
def test_gpu_graph_capture():
    _graph_capture_roundtrip(bitwise=False)


@pytest.mark.gpu
def test_gpu_no_class_qualifies():
    em, gt, es, gs, size = _layout_golden()
    gt = gt.clone()
    gt[1] = 0                    # image 0 alone: its largest class has < 1024 reduced pixels
    assert R.plan(_reduce(gt, size), _reduce(gs, size), IGN, 1024, 2, 0, 0)["header"].tolist() == [0, 0, 0, 0]
    emd, esd = _to_dev(em, grad=True), _to_dev(es, grad=True)
    crit = _crit(1024, 2)
    loss = crit(emd, gt.to(DEV), esd, gs.to(DEV))
    loss.backward()
    assert loss.dim() == 0 and float(loss.item()) == 0.0
    assert crit.last_plan()["header"].tolist() == [0, 0, 0, 0]
    assert float(emd.grad.abs().max()) == 0.0 and float(esd.grad.abs().max()) == 0.0


@pytest.mark.gpu
def test_gpu_more_classes_than_capacity():
    em, gt, es, gs, size = _layout_71()
    gm, gsd = _reduce(gt, size), _reduce(gs, size)
    emd, esd = _to_dev(em, grad=True), _to_dev(es, grad=True)
    crit = _crit(64, 5, seed=2)
    loss = crit(emd, gt.to(DEV), esd, gs.to(DEV))
    loss.backward()
    plan = _download(crit)
    ref = R.plan(gm, gsd, IGN, 64, 5, 2, 0)
    assert ref["dropped"] > 0 and plan["dropped"] == ref["dropped"]
    _assert_plan_equal(plan, ref)
    assert sorted(set(plan["labels"][:5 * 64].tolist())) == [1, 2, 3, 4, 5]
    _assert_loss_and_grads(loss, emd.grad, esd.grad, *_cpu_reference(em, es, plan))
    crit(emd, gt.to(DEV), esd, gs.to(DEV))          # the counter is cumulative
    assert int(crit.last_plan()["dropped_classes"].item()) == 2 * ref["dropped"]


@pytest.mark.gpu
def test_gpu_no_background():
    em, gt, es, gs, size = _layout_golden()
    gt = gt.clone()
    gt[gt == 0] = 255
    crit = _crit(512, 3)
    crit(em.to(DEV), gt.to(DEV), es.to(DEV), gs.to(DEV))
    plan = _download(crit)
    _assert_plan_equal(plan, R.plan(_reduce(gt, size), _reduce(gs, size), IGN, 512, 3, 0, 0))
    assert int(plan["header"][3]) == 0 and int(plan["header"][0]) == int(plan["header"][1]) == 512 * int(plan["header"][2]) > 0


@pytest.mark.gpu
def test_gpu_limits_raise():
    from cavp_amd._lib import CavpError
    from cavp_amd.contrast import ContrastLoss
    em, gt, es, gs, _ = _layout_golden()
    emd, esd, gsd = em.to(DEV), es.to(DEV), gs.to(DEV)
    with pytest.raises(CavpError):
        ContrastLoss(TEMP, IGN, 2048).use_device_sampler(2)
    with pytest.raises(CavpError):
        ContrastLoss(TEMP, IGN, 0).use_device_sampler(2)
    with pytest.raises(CavpError):
        _crit(64, 2)(emd.half(), gt.to(DEV), esd.half(), gsd)
    for bad in (300, -1):
        g2 = gt.clone()
        g2[0, 100, 100] = bad
        crit = _crit(64, 3)
        crit(emd, g2.to(DEV), esd, gsd)
        with pytest.raises(CavpError):
            crit.last_plan()
    with pytest.raises(CavpError):            # a non-uniform pixel stride (the _strides_bcp rule)
        _crit(64, 3)(emd[:, :, :, :28], gt.to(DEV), esd[:, :, :, :28], gsd)
