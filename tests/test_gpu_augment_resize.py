"""GPU tests of the resize variant of the frame augmentation (FrameAugment(resize=True), csrc/augment.hip) against
tests/golden/augment_resize.npz - what the reference's resize_flag = True train_aug / test_aug gives through PIL for recorded
draws (tools/make_golden_augment_resize.py).  Stage 192 x 64, frames (192, 64), (150, 61), (37, 29), output 24 x 72: a vertical
ratio of 8 (32 taps, above the crop variant's 12), a horizontal upscale, two tile rows, a ragged second tile column, an odd
width.

The image bar is that of tests/test_gpu_augment.py: one uint8 step in normalised units, |d| <= 1.001 / (255 * std_c) per channel.
The target is no differing value at all - the arithmetic is integer and fp64: the share of values that differ by more than 1e-5
is capped at twice the recorded share (zero), never above 1 %.  Masks are exact."""
import os

import numpy as np
import pytest
import torch

from tests import _augment_ref as R
from tests.test_augment_resize_host import GROUPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED_DIFF_SHARE = 0.0          # DESIGN.md 4q; the cap is twice this, never above 1 %
STD = np.asarray(R.STD, np.float32)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "augment_resize.npz")))


def _aug(g, s, jitter=None, seed=0, max_batch=64, resize=True, crop=None):
    from cavp_amd.augment import FrameAugment
    return FrameAugment(crop=tuple(int(v) for v in g[s + "_out"]) if crop is None else crop, mean=R.MEAN, std=R.STD,
                        scales=tuple(float(v) for v in g[s + "_scales"]), jitter=jitter, seed=seed, device=DEV, max_batch=max_batch,
                        stage=tuple(int(v) for v in g[s + "_stage"]), resize=resize)


def _staged(g, s, idx, outside=None):
    """Device staging buffers of set s for the samples idx; outside = a byte written over everything outside each h x w corner."""
    frames, masks, sizes = g[s + "_frames"][idx].copy(), g[s + "_masks"][idx].copy(), g[s + "_sizes"][idx]
    if outside is not None:
        for k, (h, w) in enumerate(sizes):
            frames[k, h:], frames[k, :, w:], masks[k, h:], masks[k, :, w:] = outside, outside, outside, outside
    return torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV), torch.from_numpy(np.ascontiguousarray(sizes)).to(DEV)


def _run(g, group, jitter=None, outside=None, evaluate=False):
    s, idx, rows = GROUPS[group], g[group + "_sample"], g[group + "_params"]
    aug = _aug(g, s, jitter=jitter, max_batch=len(idx))
    ins = _staged(g, s, idx, outside)
    out = aug.eval_(*ins) if evaluate else aug(*ins, params=torch.from_numpy(np.ascontiguousarray(rows)).to(DEV))
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


@pytest.mark.parametrize("outside", [None, 0xA5], ids=["plain", "sentinel"])
def test_every_scale_and_flip(g, outside):
    """The three frames x the three AVS scales x flip off / on; with the bytes outside each h x w corner overwritten nothing
    changes."""
    out = _run(g, "geo", outside=outside)
    _compare(out, g["geo_image"], g["geo_mask"], what="geo")
    p, rows = out.params.cpu().numpy(), g["geo_params"]
    assert np.array_equal(p[:, :2], rows[:, :2]) and (p[:, 10:12] == 0).all() and (p[:, 15] == 0).all() and (p[:, 14] == -1).all()
    for k, i in enumerate(g["geo_sample"]):
        assert tuple(p[k, 12:14]) == R.scaled_size(*(int(v) for v in g["main_sizes"][i]), R.AVS_SCALES[rows[k, 1]])


def test_coco_scales_at_the_ratio_limit(g):
    """Stage 96 x 64 under the COCO list at 1.25 and 2.0: 2 * 96 = 8 * 24."""
    _compare(_run(g, "coco"), g["coco_image"], g["coco_mask"], what="coco")


def test_identity_is_an_exact_copy(g):
    out = _run(g, "ident")
    _compare(out, g["ident_image"], g["ident_mask"], bar_steps=0.0, what="ident")
    assert np.array_equal(out.image.cpu().numpy()[0], R.normalise(g["ident_frames"][0]))
    assert np.array_equal(out.label.cpu().numpy()[0], g["ident_masks"][0].astype(np.int64))


def test_nearest_chain_16_12_9(g):
    _compare(_run(g, "chain"), g["chain_image"], g["chain_mask"], what="chain")


@pytest.mark.parametrize("outside", [None, 0x5A], ids=["plain", "sentinel"])
def test_all_jitter_orders(g, outside):
    out = _run(g, "jit", jitter=(.5, .5, .5, .25), outside=outside)
    _compare(out, g["jit_image"], g["jit_mask"], what="jitter")
    assert np.array_equal(out.params.cpu().numpy()[:, 14], g["jit_mean"])


@pytest.mark.parametrize("outside", [None, 0xA5], ids=["plain", "sentinel"])
def test_eval_resizes_every_frame(g, outside):
    _compare(_run(g, "eval", outside=outside, evaluate=True), g["eval_image"], g["eval_mask"], what="eval")


def test_draws_equal_the_crop_variant(g):
    """The same seed and offset: params[:, 0:10] (flip, scale, order, factors, hue) of the resize variant equal the crop variant's
    over three calls; the crop origin is not drawn."""
    idx = np.asarray([0, 1, 2, 1, 0, 2, 2, 1])
    ins = _staged(g, "main", idx)
    rz = _aug(g, "main", jitter=(.5, .5, .5, .25), seed=77)
    cr = _aug(g, "main", jitter=(.5, .5, .5, .25), seed=77, resize=False, crop=(24, 24))
    seen = set()
    for k in range(3):
        a, b = rz(*ins).params.cpu().numpy(), cr(*ins).params.cpu().numpy()
        assert np.array_equal(a[:, :10], b[:, :10]), k
        assert (a[:, 10:12] == 0).all() and np.array_equal(a[:, 12:14], b[:, 12:14])
        seen |= {tuple(r) for r in a[:, :2]}
    assert rz.offset() == 3 == cr.offset() and len(seen) > 3
    rz.check()


def test_constructor_refusals():
    from cavp_amd._lib import CavpError
    from cavp_amd.augment import FrameAugment
    with pytest.raises(CavpError, match="at most 8"):
        FrameAugment(crop=(24, 72), scales=R.AVS_SCALES, jitter=None, stage=(193, 64), resize=True, device=DEV)
    with pytest.raises(CavpError, match="pad_fill"):
        FrameAugment(crop=(24, 72), scales=R.AVS_SCALES, stage=(192, 64), resize=True, pad_fill=(1, 2, 3), device=DEV)
    half = FrameAugment(crop=(24, 72), scales=(0.5,), jitter=None, stage=(384, 64), resize=True, device=DEV, max_batch=1)   # 384 / 2 = 8 * 24
    ins = (torch.zeros((1, 384, 64, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 384, 64), dtype=torch.uint8, device=DEV),
           torch.tensor([[384, 64]], dtype=torch.int32, device=DEV))
    half(*ins)
    half.check()
    with pytest.raises(CavpError, match="eval_"):
        half.eval_(*ins)                                  # 384 > 8 * 24 without the scale


def test_graph_capture_replays_equal_eager_calls(g):
    """aug(...) with resize=True and jitter captured in a torch.cuda.graph: three replays are bit-identical to three eager calls
    from the same seed."""
    from cavp_amd.augment import AugResult
    idx = np.asarray([0, 1, 2, 1])
    ins = _staged(g, "main", idx)
    cap, eager = _aug(g, "main", jitter=(.5, .5, .5, .25), seed=31), _aug(g, "main", jitter=(.5, .5, .5, .25), seed=31)
    out = AugResult(len(idx), (24, 72), torch.device(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap(*ins, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cap.manual_seed(31)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap(*ins, out=out)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager(*ins)
        assert torch.equal(out.image, e.image) and torch.equal(out.label, e.label) and torch.equal(out.params, e.params), k
        assert cap.offset() == 1 + k
