"""GPU checks of cavp_amd.metrics.VideoValidation (csrc/metrics.hip: cavp_videoval_frame_stats, cavp_videoval_combine) against the
existing entry points (ops.mask_iou_stats, ops.fmeasure_hist, ops.seg_confusion), the CPU restatement tests/_videoval_ref.py and the
reference's own numbers (tests/golden/videoval.npz).  Integers are compared exactly.  A per-video score lies in [0, 1] and is the
result of at most T + 8 float32 roundings of positive terms over exact integer counts, so it is compared with (T + 8) * 2^-24."""
import os

import numpy as np
import pytest
import torch

from cavp_amd import metrics as MT
from cavp_amd import ops
from cavp_amd._lib import CavpError
from tests import _videoval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "videoval.npz")
PR = 255


def _bound(T):
    return (T + 8) * 2.0 ** -24


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a, dtype=dtype).to(DEV)


def _logits(N, C, H, W, seed, channel=1, pr_num=PR):
    """float32 logits [N, C, H, W] whose float64 softmax of `channel` keeps 1e-5 from every threshold (offending pixels are
    redrawn): the device's float32 softmax and the restatement's then fall into the same bin at every pixel.  A condition on the
    inputs, as in tools/make_golden_videoval.py."""
    rs = np.random.RandomState(seed)
    th = R.thresholds(pr_num).astype(np.float64)
    x = (rs.randn(N, C, H, W) * 2).astype(np.float32)
    for _ in range(100):
        d = x.astype(np.float64)
        e = np.exp(d - d.max(1, keepdims=True))
        p = e[:, channel] / e.sum(1)
        near = np.abs(p[..., None] - th).min(-1) < 1e-5
        if not near.any():
            return x
        n, h, w = np.nonzero(near)
        x[n, :, h, w] = (rs.randn(len(n), C) * 2).astype(np.float32)
    raise AssertionError("no draw away from the thresholds")


def _labels(B, T, H, W, seed, amax=None):
    """{0, 1} labels (80 % the prediction when given) with a sprinkle of 255; frame (0, 0) keeps a foreground pixel."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 2, size=(B, T, H, W)).astype(np.int64)
    if amax is not None:
        lab = np.where(rs.rand(B, T, H, W) < 0.8, np.minimum(amax.reshape(B, T, H, W), 1), lab)
    lab[rs.rand(B, T, H, W) < 0.03] = 255
    lab[0, 0, 0, 0] = 1
    return lab


class _Scratch:
    """The device buffers of one VideoValidation-shaped call sequence, for driving the two entry points directly."""

    def __init__(self, N, K, max_videos=16):
        self.stats = torch.zeros((N, 4), dtype=torch.int64, device=DEV)
        self.hist = torch.zeros((N, 2, PR + 1), dtype=torch.int32, device=DEV)
        self.M = torch.zeros(((K + 1) * K,), dtype=torch.int64, device=DEV)
        self.state = torch.zeros(8, dtype=torch.int64, device=DEV)
        self.J = torch.full((max_videos,), -1.0, device=DEV)
        self.F = torch.full((max_videos,), -1.0, device=DEV)
        self.th = MT.thresholds(PR, torch.device(DEV))


def _existing_entry_points(logits, lab, parts, K, th, channel=1):
    """stats / hist / M of the participating frames `parts` from the three entry points that existed before."""
    N = logits.shape[0]
    stats = torch.zeros((N, 4), dtype=torch.int64, device=DEV)
    hist = torch.zeros((N, 2, PR + 1), dtype=torch.int32, device=DEV)
    M = torch.zeros(((K + 1) * K,), dtype=torch.int64, device=DEV)
    flat = lab.reshape((N,) + tuple(lab.shape[-2:]))
    if len(parts):
        idx = torch.as_tensor(parts, device=DEV)
        x, y = logits[idx].contiguous(), flat[idx].contiguous()
        stats[idx] = ops.mask_iou_stats(x.argmax(1), y, torch.zeros((len(parts), 4), dtype=torch.int64, device=DEV))
        hist[idx] = ops.fmeasure_hist(x, y, th, torch.zeros((len(parts), 2, PR + 1), dtype=torch.int32, device=DEV), channel)
        ops.seg_confusion(x, y, K, 255, M)
    return stats, hist, M


# ---- integers against the existing entry points and the restatement --------------------------------------------------------------
@pytest.mark.parametrize("BT", [(1, 1), (2, 3), (3, 5)])
@pytest.mark.parametrize("CK", [(2, 2), (2, 5), (3, 3), (3, 5)])
@pytest.mark.parametrize("hw", [(7, 9), (24, 28), (33, 40)])
def test_sweep(hw, CK, BT):
    (H, W), (C, K), (B, T) = hw, CK, BT
    N = B * T
    x_host = _logits(N, C, H, W, seed=100 * C + K + B)
    labels = _labels(B, T, H, W, seed=7 + B, amax=x_host.argmax(1))
    x, lab = _dev(x_host), _dev(labels)
    for count, dtype in ((None, None), ([T, 1, 0][:B], torch.int32), ([T + 2, -1, 1][:B], torch.int64)):
        ref = R.video_validation(x_host, labels, count, K)
        cnt = None if count is None else _dev(count, dtype)
        s = _Scratch(N, K)
        ops.videoval_frame_stats(x, lab, cnt, T, K, 255, s.th, s.stats, s.hist, s.M, s.state)
        clamped = [T] * B if count is None else [min(max(c, 0), T) for c in count]
        parts = [b * T + t for b in range(B) for t in range(clamped[b])]
        stats, hist, M = _existing_entry_points(x, lab, parts, K, s.th)
        assert torch.equal(s.stats, stats) and torch.equal(s.hist, hist) and torch.equal(s.M, M)
        np.testing.assert_array_equal(s.stats.cpu().numpy(), ref["stats"])
        np.testing.assert_array_equal(s.hist.cpu().numpy(), ref["hist"])
        np.testing.assert_array_equal(s.M.cpu().numpy().reshape(K + 1, K), ref["M"])
        ops.videoval_combine(s.stats, s.hist, cnt, B, T, H * W, PR, s.J, s.F, s.state)
        assert s.state.cpu().tolist() == ref["state"]
        assert int(s.stats.ne(0).sum()) == 0 and int(s.hist.ne(0).sum()) == 0          # the scratch is zero at rest
        n = len(ref["J"])
        J, F = s.J.cpu().numpy(), s.F.cpu().numpy()
        print(hw, CK, BT, count, "J", J[:n], ref["J"], "F", F[:n], ref["F"])
        assert n == sum(c > 0 for c in clamped) and (J[n:] == -1).all() and (F[n:] == -1).all()
        # with C = 3 the predicted class 2 makes sum p*t exceed the union of a {0, 1} target: J lies in [0, 2), one more binade
        np.testing.assert_allclose(J[:n], np.array(ref["J"], np.float32), rtol=0, atol=_bound(T) * (1 if C == 2 else 2))
        np.testing.assert_allclose(F[:n], np.array(ref["F"], np.float32), rtol=0, atol=_bound(T))


def test_misaligned_and_wide_logits():
    """The element path on whole quads (a base one float past a 16-byte boundary), and C = 6 > 4: the channels are loaded a second
    time for the softmax; K = 130: the confusion counts go straight to global memory."""
    B, T, H, W = 2, 2, 8, 12
    N = B * T
    for C, K, shift in ((2, 2, True), (6, 6, False), (6, 130, True)):
        x_host = _logits(N, C, H, W, seed=C + K)
        labels = _labels(B, T, H, W, seed=3)
        labels[1, 1, 2, :5] = [K, K + 1, 1000, -1, -7]                     # rows K and "not counted", all of them outside {0, 1, 255}
        buf = torch.empty(x_host.size + 1, device=DEV)
        x = (buf[1:] if shift else buf[:-1]).view(N, C, H, W).copy_(_dev(x_host))
        assert (x.data_ptr() % 16 != 0) == shift
        lab = _dev(labels)
        ref = R.video_validation(x_host, labels, None, K)
        s = _Scratch(N, K)
        ops.videoval_frame_stats(x, lab, None, T, K, 255, s.th, s.stats, s.hist, s.M, s.state)
        stats, hist, M = _existing_entry_points(x, lab, list(range(N)), K, s.th)
        assert torch.equal(s.stats, stats) and torch.equal(s.hist, hist) and torch.equal(s.M, M)
        np.testing.assert_array_equal(s.hist.cpu().numpy(), ref["hist"])
        np.testing.assert_array_equal(s.M.cpu().numpy().reshape(K + 1, K), ref["M"])
        assert s.state.cpu().tolist()[:4] == [5, 0, 0, 0] == ref["state"][:4]


@pytest.mark.parametrize("pr_num", [1, 7, 300])
def test_other_threshold_counts(pr_num):
    """Fewer thresholds than a wave has lanes, and more than a workgroup has threads (five bins per lane in the combine's scan)."""
    B, T, C, K, H, W = 2, 5, 2, 2, 7, 9
    x_host = _logits(B * T, C, H, W, seed=pr_num, pr_num=pr_num)
    labels = _labels(B, T, H, W, seed=pr_num + 1, amax=x_host.argmax(1))
    labels[1, 2] = 0                                                        # a skipped frame
    ref = R.video_validation(x_host, labels, None, K, pr_num=pr_num)
    vv = MT.VideoValidation(num_classes=K, pr_num=pr_num, max_frames=B * T, max_videos=4, device=DEV)
    x, lab = _dev(x_host), _dev(labels)
    ops.videoval_frame_stats(x, lab, None, T, K, 255, MT.thresholds(pr_num, torch.device(DEV)), *_fresh(vv))
    np.testing.assert_array_equal(vv._hist.cpu().numpy(), ref["hist"])
    hist = ops.fmeasure_hist(x, lab.flatten(0, 1), vv._th, torch.zeros_like(vv._hist))
    assert torch.equal(vv._hist, hist)
    ops.videoval_combine(vv._stats, vv._hist, None, B, T, H * W, pr_num, vv._J, vv._F, vv._state)
    J, F = (t.cpu().numpy() for t in vv.video_scores())
    print(pr_num, "J", J, ref["J"], "F", F, ref["F"])
    np.testing.assert_allclose(J, np.array(ref["J"], np.float32), rtol=0, atol=_bound(T))
    np.testing.assert_allclose(F, np.array(ref["F"], np.float32), rtol=0, atol=_bound(T))
    assert int(vv._stats.ne(0).sum()) == 0 and int(vv._hist.ne(0).sum()) == 0


def _fresh(vv):
    """Allocate vv's device buffers without an update: (stats, hist, M, state) for a direct call of the frame entry point."""
    vv._ensure()
    return vv._stats, vv._hist, vv._counts, vv._state


def test_mask_form_guards():
    """A mask byte >= K sets no confusion bin and is counted; the planes are read as they are."""
    B, T, H, W, K = 1, 2, 8, 12, 3
    rs = np.random.RandomState(0)
    mask = rs.randint(0, K, size=(2, H, W)).astype(np.uint8)
    mask[0, 0, :3] = [K, 200, 255]
    prob = (np.round(rs.rand(2, H, W) * 1024) / 1024).astype(np.float32)    # k / 1024: exact in both searches
    prob[1, 0, :3] = [0.0, 1.0, np.nan]                                      # a NaN lands in bin 0
    labels = _labels(B, T, H, W, seed=1)
    ref = R.video_validation(mask, labels, None, K, prob=prob)
    assert ref["state"][1] == 3
    s = _Scratch(2, K)
    ops.videoval_frame_stats(_dev(mask), _dev(labels), None, T, K, 255, s.th, s.stats, s.hist, s.M, s.state, prob=_dev(prob))
    np.testing.assert_array_equal(s.stats.cpu().numpy(), ref["stats"])
    np.testing.assert_array_equal(s.hist.cpu().numpy(), ref["hist"])
    np.testing.assert_array_equal(s.M.cpu().numpy().reshape(K + 1, K), ref["M"])
    hist = ops.fmeasure_hist(_dev(prob), _dev(labels[0]), s.th, torch.zeros((2, 2, PR + 1), dtype=torch.int32, device=DEV))
    assert torch.equal(s.hist, hist)
    stats = ops.mask_iou_stats(_dev(mask).long(), _dev(labels[0]), torch.zeros((2, 4), dtype=torch.int64, device=DEV))
    assert torch.equal(s.stats, stats)
    ops.videoval_combine(s.stats, s.hist, None, B, T, H * W, PR, s.J, s.F, s.state)
    assert s.state.cpu().tolist() == ref["state"]


def test_frames_that_take_no_part_are_not_read():
    B, T, C, K, H, W = 3, 5, 2, 2, 24, 28
    x_host = _logits(B * T, C, H, W, seed=5)
    labels = _labels(B, T, H, W, seed=6, amax=x_host.argmax(1))
    count = [T, 1, 0]
    got = []
    for poison in (False, True):
        xh, lh = x_host.copy().reshape(B, T, C, H, W), labels.copy()
        if poison:
            for b in range(B):
                xh[b, count[b]:] = np.nan
                lh[b, count[b]:] = 10 ** 6
        vv = MT.VideoValidation(num_classes=K, max_frames=B * T, max_videos=8, device=DEV)
        vv.update(_dev(xh.reshape(B * T, C, H, W)), _dev(lh), _dev(count, torch.int32))
        vv.check()                                                          # no label outside {0, 1, 255} was seen
        J, F = vv.video_scores()
        got.append((J.cpu(), F.cpu(), vv.counts().cpu(), vv._state.cpu()))
    assert got[0][0].numel() == 2
    for a, b in zip(*got):
        assert torch.equal(a, b)


# ---- the reference's numbers -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", ["vec", "sca"])
@pytest.mark.parametrize("split", [False, True])
def test_fixture(z, name, split):
    logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
    B, T = labels.shape[:2]
    x, lab = _dev(logits), _dev(labels)
    vv = MT.VideoValidation(num_classes=2, max_frames=B * T, max_videos=8, device=DEV)
    for sl in ([slice(0, 1), slice(1, B)] if split else [slice(0, B)]):
        vv.update(x[sl].flatten(0, 1), lab[sl], None if split else _dev([T] * B, torch.int64))
    np.testing.assert_array_equal(vv.counts().cpu().numpy(), z[f"{name}_M"])
    J, F = (t.cpu().numpy().astype(np.float64) for t in vv.video_scores())
    means = vv.video_means()
    print(name, "J", J, z[f"{name}_J"], "F", F, z[f"{name}_F"], "means", means, z[f"{name}_means"])
    np.testing.assert_allclose(J, z[f"{name}_J"].astype(np.float64), rtol=0, atol=_bound(T))
    np.testing.assert_allclose(F, z[f"{name}_F"], rtol=0, atol=_bound(T))
    np.testing.assert_allclose(means, z[f"{name}_means"], rtol=0, atol=_bound(T))
    pair, perf = vv.results()
    assert [float(v) for v in pair] == z[f"{name}_rounded"].tolist()
    assert [float(v) for v in perf] == z[f"{name}_perf"].tolist()
    assert [float(v) for v in MT.get_performance(vv.miou, vv.fg)] == z[f"{name}_perf"].tolist()
    assert vv.miou.counts().data_ptr() == vv.counts().data_ptr()                    # the accessors read, they do not copy
    assert torch.equal(lab.cpu(), torch.from_numpy(labels))                         # the labels are never written
    assert int(vv._stats.ne(0).sum()) == 0 and int(vv._hist.ne(0).sum()) == 0
    vv.check()


# ---- update_lowres ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw", [(24, 28), (7, 9)])
def test_update_lowres_equals_update_on_the_upsample(hw, dtype):
    B, T, C, K = 2, 3, 2, 2
    (H, W), N = hw, 6
    g = torch.Generator().manual_seed(H)
    lo = (torch.randn((N, (H + 3) // 4, (W + 3) // 4, C), generator=g) * 2).to(dtype).to(DEV)
    full = ops.bilinear_to_nchw(lo, torch.empty((N, C, H, W), dtype=torch.float32, device=DEV), False)
    labels = _dev(_labels(B, T, H, W, seed=2, amax=full.argmax(1).cpu().numpy()))
    count = _dev([T, 2], torch.int32)
    a = MT.VideoValidation(num_classes=K, max_frames=N, max_videos=4, device=DEV)
    b = MT.VideoValidation(num_classes=K, max_frames=N, max_videos=4, device=DEV)
    for _ in range(2):
        a.update(full, labels, count)
        b.update_lowres(lo, labels, count, input_shape=(H, W))
    assert torch.equal(a._res, b._res)                 # counts, state words and the J | F bits in one buffer
    assert a.videos() == 4 and int(a.counts().sum()) > 0
    assert int(b._stats.ne(0).sum()) == 0 and int(b._hist.ne(0).sum()) == 0


# ---- accumulation, overflow, reset -----------------------------------------------------------------------------------------------
def test_two_updates_equal_one_update_of_the_concatenation():
    B, T, C, K, H, W = 4, 3, 2, 2, 7, 9
    x_host = _logits(B * T, C, H, W, seed=21)
    labels = _labels(B, T, H, W, seed=22, amax=x_host.argmax(1))
    count = [T, 0, 2, 1]
    x, lab, cnt = _dev(x_host).view(B, T, C, H, W), _dev(labels), _dev(count, torch.int32)
    one = MT.VideoValidation(num_classes=K, max_frames=B * T, max_videos=8, device=DEV)
    one.update(x.flatten(0, 1), lab, cnt)
    two = MT.VideoValidation(num_classes=K, max_frames=B * T, max_videos=8, device=DEV)
    two.update(x[:1].flatten(0, 1), lab[:1], cnt[:1])
    two.update(x[1:].flatten(0, 1), lab[1:], cnt[1:])
    assert torch.equal(one._res, two._res) and one.videos() == 3
    ra, rb = one.results(), two.results()
    assert [float(v) for v in ra[0] + ra[1]] == [float(v) for v in rb[0] + rb[1]]
    ref = R.video_validation(x_host, labels, count, K)
    np.testing.assert_array_equal(one.counts().cpu().numpy(), ref["M"])
    np.testing.assert_allclose(one.video_scores()[0].cpu().numpy(), np.array(ref["J"], np.float32), rtol=0, atol=_bound(T))
    np.testing.assert_allclose(one.video_scores()[1].cpu().numpy(), np.array(ref["F"], np.float32), rtol=0, atol=_bound(T))


def test_max_videos_overflow_and_reset():
    B, T, C, K, H, W = 3, 2, 2, 2, 7, 9
    x_host = _logits(B * T, C, H, W, seed=31)
    labels = _labels(B, T, H, W, seed=32, amax=x_host.argmax(1))
    x, lab = _dev(x_host), _dev(labels)
    vv = MT.VideoValidation(num_classes=K, max_frames=B * T, max_videos=4, device=DEV)
    vv.update(x, lab)
    first = tuple(t.clone() for t in vv.video_scores())
    vv.check()
    vv.update(x, lab)                                                       # videos 3, 4, 5: only one more slot
    assert vv.videos() == 4
    J, F = vv.video_scores()
    assert torch.equal(J[:3], first[0]) and torch.equal(F[:3], first[1])    # the earlier slots are intact
    assert J[3] == first[0][0] and F[3] == first[1][0]
    with pytest.raises(CavpError, match="2 video"):
        vv.check()
    vv.check()                                                              # the counters were cleared by the raising check
    with pytest.raises(CavpError, match="count"):
        vv.update(x, lab, _dev([T + 1, 0, -3], torch.int64))
        vv.check()
    vv.reset()
    assert vv.videos() == 0 and int(vv.counts().sum()) == 0 and vv.video_scores()[0].numel() == 0
    with pytest.raises(CavpError, match="no video"):
        vv.results()
    vv.update(x, lab)
    assert torch.equal(vv.video_scores()[0], first[0]) and torch.equal(vv.video_scores()[1], first[1])
    vv.check()


# ---- no sync: graph capture ------------------------------------------------------------------------------------------------------
def test_update_captured_in_a_graph():
    from cavp_amd.train import _no_gc_during_capture
    B, T, C, K, H, W = 3, 5, 2, 2, 24, 28
    xs = [_dev(_logits(B * T, C, H, W, seed=41 + i)) for i in range(2)]
    labs = [_dev(_labels(B, T, H, W, seed=51 + i, amax=xs[i].argmax(1).cpu().numpy())) for i in range(2)]
    cnts = [_dev([T, 0, 3], torch.int32), _dev([2, T, 1], torch.int32)]

    eager = MT.VideoValidation(num_classes=K, max_frames=B * T, max_videos=8, device=DEV)
    for i in range(2):
        eager.update(xs[i], labs[i], cnts[i])
    assert eager.videos() == 5

    vv = MT.VideoValidation(num_classes=K, max_frames=B * T, max_videos=8, device=DEV)
    x, lab, cnt = xs[0].clone(), labs[0].clone(), cnts[0].clone()           # the static buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vv.update(x, lab, cnt)             # the first call allocates: it cannot be the captured one
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        vv.update(x, lab, cnt)
    vv.reset()
    assert vv.videos() == 0
    for i in range(2):
        x.copy_(xs[i]), lab.copy_(labs[i]), cnt.copy_(cnts[i])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(vv._res, eager._res)
    assert int(vv._stats.ne(0).sum()) == 0 and int(vv._hist.ne(0).sum()) == 0
    vv.check()

