"""GPU tests of the frame augmentation (cavp_amd/augment.py, csrc/augment.hip) against tests/golden/augment.npz - what the
reference's train_aug gives through PIL for recorded draws (tools/make_golden_augment.py) - and against the numpy restatement.
Stage 48 x 64, samples (29, 37), (40, 56), (48, 64), (13, 60): a width not divisible by 4, 4/3 ties, a full slot, one side below
the crop.

The image bar: one uint8 step in normalised units, |d| <= 1.001 / (255 * std_c) per channel - a bicubic coefficient that differs
in its last bit can move a byte of the horizontal pass by one, and the vertical pass carries it on with a weight of about 1.
The target is no differing pixel at all: the share of values that differ by more than 1e-5 is asserted to be the recorded share
(zero), which keeps the one-step bar from hiding a regression."""
import os

import numpy as np
import pytest
import torch

from tests import _augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED_DIFF_SHARE = 0.0          # DESIGN.md 4p; the cap is twice this, never above 1 %
STD = np.asarray(R.STD, np.float32)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "augment.npz")))


def _aug(crop, jitter=None, scales=R.COCO_SCALES, seed=0, max_batch=64, stage=(48, 64)):
    from cavp_amd.augment import FrameAugment
    return FrameAugment(crop=crop, mean=R.MEAN, std=R.STD, scales=scales, jitter=jitter, seed=seed, device=DEV, max_batch=max_batch,
                        stage=stage)


def _staged(g, idx, outside=None):
    """Device staging buffers for the samples idx; outside = a byte value written over everything outside each h x w corner."""
    frames, masks, sizes = g["frames"][idx].copy(), g["masks"][idx].copy(), g["sizes"][idx]
    if outside is not None:
        for k, (h, w) in enumerate(sizes):
            frames[k, h:], frames[k, :, w:], masks[k, h:], masks[k, :, w:] = outside, outside, outside, outside
    return torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV), torch.from_numpy(np.ascontiguousarray(sizes)).to(DEV)


def _run(g, prefix, jitter=None, outside=None, scales=R.COCO_SCALES, keep=None):
    idx, rows = g[prefix + "_sample"], g[prefix + "_params"]
    if keep is not None:
        idx, rows = idx[keep], rows[keep]
    aug = _aug(tuple(int(v) for v in g[prefix + "_crop"]), jitter=jitter, scales=scales, max_batch=len(idx))
    out = aug(*_staged(g, idx, outside), params=torch.from_numpy(np.ascontiguousarray(rows)).to(DEV))
    aug.check()
    return out


def _compare(out, want_u8, want_mask, bar_steps=1.001, share_cap=2 * RECORDED_DIFF_SHARE, what=""):
    got = out.image.cpu().numpy()
    want = np.stack([R.normalise(im) for im in want_u8])
    d = np.abs(got - want)
    steps = float((d * (255.0 * STD)[None, :, None, None]).max())
    share = float((d > 1e-5).mean())
    print(f"{what}: largest difference {steps:.4f} uint8 steps, share of values off by more than 1e-5: {share:.6f}")
    assert np.array_equal(out.label.cpu().numpy(), want_mask.astype(np.int64)), f"{what}: mask"
    assert (d <= bar_steps / (255.0 * STD)[None, :, None, None]).all(), f"{what}: {steps} steps"
    assert share <= min(share_cap, 0.01), f"{what}: share {share}"


# ------------------------------------------------------------------------------------------------------------------ 1 geometry
def test_geometry_every_scale_flip_and_origin(g):
    """Crop 16 x 24 (non-square: swapped axes show), no jitter, every scale of the COCO list, flip off and on, origins 0 / maximum
    / interior: the mask exactly, the image inside one uint8 step with no differing value."""
    rows = g["geo_params"]
    assert set(rows[:, 1]) == set(range(7)) and set(rows[:, 0]) == {0, 1}
    assert (rows[:, 10] == 0).any() and (rows[:, 11] == 0).any() and (rows[:, 10] > 0).any() and (rows[:, 11] > 0).any()
    out = _run(g, "geo")
    _compare(out, g["geo_image"], g["geo_mask"], what="geometry")
    p = out.params.cpu().numpy()
    assert np.array_equal(p[:, [0, 1, 10, 11]], rows[:, [0, 1, 10, 11]]) and (p[:, 15] == 0).all() and (p[:, 14] == -1).all()
    for k, i in enumerate(g["geo_sample"]):
        assert tuple(p[k, 12:14]) == R.scaled_size(*(int(v) for v in g["sizes"][i]), R.COCO_SCALES[rows[k, 1]])


def test_geometry_avs_scale_list(g):
    """The "avs" set-up: scales (0.5, 0.75, 1.0), no jitter - the cases of the fixture that use those three scales."""
    keep = np.flatnonzero(g["geo_params"][:, 1] < 3)
    assert len(keep) >= 12
    out = _run(g, "geo", scales=R.AVS_SCALES, keep=keep)
    _compare(out, g["geo_image"][keep], g["geo_mask"][keep], what="avs list")


# ------------------------------------------------------------------------------------------------------------------------ 2 pad
def test_pad_fill_and_literal_rule(g):
    """Crop 32 x 32 on (13, 60) and (29, 37) at 0.5 and 1.0: the fixture, and every padded pixel exactly (pad_fill / 255 - mean) /
    std with the mask 255."""
    out = _run(g, "pad")
    _compare(out, g["pad_image"], g["pad_mask"], what="pad")
    fill = R.normalise(np.asarray(g["pad_fill"], np.uint8)[None, None, :])[:, 0, 0]
    img, lbl, p = out.image.cpu().numpy(), out.label.cpu().numpy(), out.params.cpu().numpy()
    seen = 0
    for k in range(len(p)):
        top, left, sh, sw = (int(p[k, c]) for c in (10, 11, 12, 13))
        yy, xx = np.mgrid[0:32, 0:32]
        padded = (yy + top >= sh) | (xx + left >= sw)
        seen += int(padded.sum())
        assert (lbl[k][padded] == 255).all()
        for c in range(3):
            assert (img[k, c][padded] == fill[c]).all()
    assert seen > 1000


def test_sample_that_cannot_hold_the_crop_is_counted(g):
    """(29, 37) at 0.5 is 14 x 18; for the 16 x 24 crop the literal rule pads the bottom by 24 - 14 and the right by max(16 - 18, 0)
    = 0: 24 x 18 cannot hold 16 x 24 and torchvision raises.  The call returns normally, check() raises, then is clean again."""
    from cavp_amd._lib import CavpError
    idx, rows = g["bad_sample"], g["bad_params"]
    aug = _aug(tuple(int(v) for v in g["geo_crop"]), max_batch=len(idx))
    out = aug(*_staged(g, idx), params=torch.from_numpy(rows).to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(out.image).all() and (out.params[:, 15] != 0).all()
    with pytest.raises(CavpError, match="cannot hold the crop"):
        aug.check()
    aug.check()
    # a staged size outside the slot and a params field out of range are counted too, and rendered from clamped values
    frames, masks, sizes = _staged(g, np.asarray([1, 1, 1]))
    sizes[0, 0], sizes[1, 1] = 49, 0
    rows = np.stack([R.params_row(0, 2, 0, 0), R.params_row(0, 2, 0, 0), R.params_row(0, 7, 999, -3)])
    aug = _aug((16, 24), max_batch=3)
    out = aug(frames, masks, sizes, params=torch.from_numpy(rows).to(DEV))
    torch.cuda.synchronize()
    assert out.params[:, 15].tolist() == [1, 1, 1]
    with pytest.raises(CavpError, match="3 sample"):
        aug.check()


# --------------------------------------------------------------------------------------------------------------------- 3 jitter
def test_jitter_every_operation_order(g):
    """B = 24, one sample per order of the four operations, (40, 56) at 1.25, crop 32 x 32, factors at the clamping ends, hue
    shifts 0, 63 and 231: the bar of the geometry test (the hue path meets it: DESIGN.md 4p), and the contrast degenerate the
    kernel used is the reference's integer."""
    rows = g["jit_params"]
    assert len({tuple(r[2:6]) for r in rows}) == 24 and set(rows[:, 9]) == {0, 63, 231}
    out = _run(g, "jit", jitter=(.5, .5, .5, .25))
    assert np.array_equal(out.params[:, 14].cpu().numpy(), g["jit_mean"])
    _compare(out, g["jit_image"], g["jit_mask"], what="jitter")


# ---------------------------------------------------------------------------------------------------------------------- 4 draws
def test_draws_are_in_range_and_uniform():
    B = 1024
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 256, (B, 48, 64, 3), dtype=np.uint8)).to(DEV)
    masks = torch.zeros((B, 48, 64), dtype=torch.uint8, device=DEV)
    sizes = torch.tensor([[40, 56]] * B, dtype=torch.int32, device=DEV)
    aug = _aug((16, 24), jitter=(.5, .5, .5, .25), seed=77, max_batch=B)
    first = aug(frames, masks, sizes)
    p = first.params.cpu().numpy()
    fac = first.factors().cpu().numpy()
    second = aug(frames, masks, sizes).params.cpu().numpy()
    aug.check()
    assert aug.offset() == 2 and not np.array_equal(p, second)
    aug.manual_seed(77)
    assert np.array_equal(aug(frames, masks, sizes).params.cpu().numpy(), p)
    # ranges
    assert set(p[:, 0]) == {0, 1} and p[:, 1].min() == 0 and p[:, 1].max() == 6
    assert (np.sort(p[:, 2:6], axis=1) == np.arange(4)).all()
    assert (fac >= 0.5).all() and (fac <= 1.5).all() and fac.std(0).min() > 0.2
    hue = p[:, 9].astype(np.int64)
    signed = np.where(hue > 127, hue - 256, hue)
    assert (np.abs(signed) <= 63).all() and signed.min() < -50 and signed.max() > 50     # trunc(255 * U[-0.25, 0.25])
    sh, sw = p[:, 12], p[:, 13]
    assert all((sh[k], sw[k]) == R.scaled_size(40, 56, R.COCO_SCALES[p[k, 1]]) for k in range(B))
    assert (p[:, 10] >= 0).all() and (p[:, 10] <= sh - 16).all() and (p[:, 11] >= 0).all() and (p[:, 11] <= sw - 24).all()
    assert (p[:, 10] == 0).any() and (p[:, 10] == sh - 16).any() and (p[:, 11] == 0).any() and (p[:, 11] == sw - 24).any()
    assert (p[:, 15] == 0).all()
    # 4 sigma of the binomial
    def within(count, prob):
        return abs(count - B * prob) <= 4.0 * np.sqrt(B * prob * (1.0 - prob))
    assert within(int(p[:, 0].sum()), 0.5)
    assert all(within(int((p[:, 1] == s).sum()), 1 / 7) for s in range(7))
    code = p[:, 2] * 64 + p[:, 3] * 16 + p[:, 4] * 4 + p[:, 5]
    counts = np.unique(code, return_counts=True)[1]
    assert len(counts) == 24 and all(within(int(c), 1 / 24) for c in counts)


# -------------------------------------------------------------------------------------------------------------------- 5 capture
def test_graph_capture_replays_equal_eager_calls(g):
    """aug(...) captured in a torch.cuda.graph (capture raises if anything synchronises): three replays are bit-identical to three
    eager calls from the same seed, and the offset advances by three."""
    from cavp_amd.augment import AugResult
    idx = np.asarray([0, 1, 2, 3, 1, 2])
    ins = _staged(g, idx)
    cap, eager = _aug((16, 24), jitter=(.5, .5, .5, .25), seed=31), _aug((16, 24), jitter=(.5, .5, .5, .25), seed=31)
    out = AugResult(len(idx), (16, 24), torch.device(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap(*ins, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cap.manual_seed(31)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap(*ins, out=out)                       # (recorded, not run: the offset is still 0)
    tables = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager(*ins)
        assert torch.equal(out.image, e.image) and torch.equal(out.label, e.label) and torch.equal(out.params, e.params), k
        assert cap.offset() == 1 + k
        tables.append(out.params.cpu().numpy().copy())
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])


def test_prologue_of_the_captured_train_step(deterministic):
    """The augmentation as the `prologue` of capture_train_step on the smallest configuration of the capture tests (B = 4, 64 x 64,
    three classes; fixed-order reductions, so that a replay is bit-identical to the eager step as in
    test_deterministic_mode_is_bit_reproducible): the replayed loss equals eager aug + train_step from the same state."""
    from cavp_amd.augment import AugResult
    from cavp_amd.synth import synth_inputs
    from tests.test_gpu_train_model import _build
    cfg = dict(C=3, B=4, hw=(64, 64), lds=[False, False, False])
    B, seed = cfg["B"], 1234
    image, audio, label = [t.to(DEV) for t in synth_inputs(B, cfg["hw"], audio_batch=2 * B, num_classes=cfg["C"], seed=2)]
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (B, 80, 96, 3), dtype=np.uint8)).to(DEV)
    mk = np.zeros((B, 80, 96), np.uint8)
    mk[:, 10:50, 20:70], mk[:, 40:70, 5:40], mk[:, :3] = 1, 2, 255
    masks = torch.from_numpy(mk).to(DEV)
    sizes = torch.tensor([[80, 96], [70, 90], [66, 71], [75, 96]], dtype=torch.int32, device=DEV)

    def aug_of(s):
        return _aug((64, 64), jitter=(.5, .5, .5, .25), seed=s, max_batch=B, stage=(80, 96))

    m, sd = _build(cfg)
    stats = {k: v for k, v in sd.items() if "running_" in k or "num_batches" in k}
    e = aug_of(seed)(frames, masks, sizes)
    l1 = m.train_step(e.image, audio, e.label, all_reduce=False).clone()
    torch.cuda.synchronize()
    aug = aug_of(0)
    res = AugResult(B, (64, 64), torch.device(DEV))

    def prologue():
        aug(frames, masks, sizes, out=res)
        image.copy_(res.image)
        label.copy_(res.label)

    replay = m.capture_train_step(image, audio, label, prologue=prologue)
    m.load_state_dict(stats, strict=False)
    aug.manual_seed(seed)
    l2 = replay().clone()
    torch.cuda.synchronize()
    aug.check()
    print(f"prologue: eager {float(l1):.6f}, replay {float(l2):.6f}")
    assert torch.equal(res.image, e.image) and torch.equal(res.label, e.label) and torch.equal(res.params, e.params)
    assert torch.equal(l1, l2)
    assert aug.offset() == 1


# ---------------------------------------------------------------------------------------------------------------------- 6 eval_
def test_eval_is_totensor_normalize_of_the_window(g):
    """ToTensor + Normalize as the reference computes them on the CPU: true float32 divisions (tests/_augment_ref.normalise)."""
    idx = np.asarray([0, 1, 2])
    aug = _aug((16, 24), jitter=(.5, .5, .5, .25))
    out = aug.eval_(*_staged(g, idx))
    aug.check()
    want = np.stack([R.normalise(g["frames"][i, :16, :24]) for i in idx])
    assert np.array_equal(out.image.cpu().numpy(), want)
    assert np.array_equal(out.label.cpu().numpy(), g["masks"][idx][:, :16, :24].astype(np.int64))
    assert aug.offset() == 1


# ------------------------------------------------------------------------------------------------------------- 7 out of bounds
@pytest.mark.parametrize("prefix,jitter", [("geo", None), ("pad", None), ("jit", (.5, .5, .5, .25))])
def test_bytes_outside_the_corner_are_never_read(g, prefix, jitter):
    a = _run(g, prefix, jitter=jitter, outside=0xFF)
    b = _run(g, prefix, jitter=jitter, outside=0x00)
    assert torch.equal(a.image, b.image) and torch.equal(a.label, b.label) and torch.equal(a.params, b.params)
    _compare(a, g[prefix + "_image"], g[prefix + "_mask"], what=f"outside bytes, {prefix}")
