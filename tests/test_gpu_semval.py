"""GPU checks of cavp_amd.metrics.SemanticValidation (csrc/metrics.hip: cavp_semval_frame_counts, cavp_semval_combine) against the
CPU restatement tests/_semval_ref.py and the reference's own numbers (tests/golden/semval.npz).

Bounds: the integer counts are compared exactly.  Every float32 result of the device is compared BIT FOR BIT with the restatement:
both perform the same IEEE single-precision operations on the same exact integers in the same order (frames ascending, classes
ascending), so there is no rounding to allow for; a NaN (a frame without a non-zero IoU) must be a NaN.  Against the reference's
stored outputs ious / fscores / cls_count are bit-equal as well; frame_miou and the binary value are within 4 float32 ulp, because
the reference's torch.sum does not add in ascending order (at most 5 positive terms in the fixture)."""
import os

import numpy as np
import pytest
import torch

from cavp_amd import metrics as MT
from cavp_amd import ops
from cavp_amd._lib import CavpError
from tests import _semval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "semval.npz")


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a, dtype=dtype).to(DEV)


def _bits(got, want):
    """Bit equality of float32 arrays; a NaN matches a NaN of any payload."""
    got = np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got, np.float32)
    want = np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def _ulp(got, want, ulp=4):
    got, want = np.atleast_1d(np.asarray(got, np.float32)), np.atleast_1d(np.asarray(want, np.float32))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) <= ulp * np.spacing(np.abs(want[ok])).astype(np.float64)).all(), \
        (got, want)


def _inputs(B, T, K, H, W, seed):
    """float32 logits [B*T, K, H, W] and int64 labels [B, T, H, W]: 70 % the prediction, the rest any class, a sprinkle of 255, -1
    and K + 2; frame (0, 0) of a batch with more than one frame is all background in label and prediction."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B * T, K, H, W) * 2).astype(np.float32)
    if B * T > 1:
        x[0, 0] = 50.0
    amax = x.argmax(1).reshape(B, T, H, W)
    lab = np.where(rs.rand(B, T, H, W) < 0.7, amax, rs.randint(0, K, size=(B, T, H, W))).astype(np.int64)
    r = rs.rand(B, T, H, W)
    lab[r < 0.03] = 255
    lab[(r >= 0.03) & (r < 0.05)] = -1
    lab[(r >= 0.05) & (r < 0.07)] = K + 2
    if B * T > 1:
        lab[0, 0] = 0
    return x, lab


def _frame_counts(pred, lab, cnt, B, T, K):
    """The integer scratch [B*T, 3K + 4] of the frame entry point alone, and its state words."""
    N, hw = B * T, lab.shape[-1] * lab.shape[-2]
    scratch = torch.zeros((N, 3 * K + 4), dtype=torch.int32, device=DEV)
    state = torch.zeros(ops.SEMVAL_STATE_WORDS, dtype=torch.int64, device=DEV)
    acc = torch.zeros(3 * K + 1, device=DEV)
    last = torch.zeros(3 * K + 1 + 2 * N, device=DEV)
    is_mask = pred.dtype == torch.uint8
    ops.semval_update(pred, is_mask, lab, cnt, B, T, 0 if is_mask else K, hw, K, N, scratch, acc, last, state, combine=False)
    assert int(acc.ne(0).sum()) == 0 and int(last.ne(0).sum()) == 0
    return scratch.cpu().numpy().astype(np.int64), state.cpu().tolist()


def _check_call(sv, ref, acc):
    """The last call of `sv` against the restatement's call `ref`, the running state against the Accumulator `acc`."""
    K, N = sv.num_classes, len(ref["frame_miou"])
    ious, fscores, cls_count, frame_miou = sv.last_call()
    _bits(ious, ref["ious"]), _bits(fscores, ref["fscores"]), _bits(cls_count, ref["cls_count"]), _bits(frame_miou, ref["frame_miou"])
    _bits(sv._last[3 * K], ref["binary"])
    _bits(sv.accumulators(), acc.accumulators())
    _bits(sv._acc[3 * K], acc.binary)
    assert sv.frames() == acc.frames and N == sv._last_frames
    assert int(sv._scratch.ne(0).sum()) == 0                                      # the scratch is zero at rest
    assert int(sv._state[3]) == 0                                                 # and so is the ticket


# ---- counts and float tail against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("BT", [(1, 1), (2, 3), (3, 5)])
@pytest.mark.parametrize("K", [2, 5, 71, 130])
@pytest.mark.parametrize("hw", [(7, 9), (24, 28), (33, 40)])
def test_sweep(hw, K, BT):
    (H, W), (B, T) = hw, BT
    x_host, labels = _inputs(B, T, K, H, W, seed=1000 * K + 10 * B + H)
    x, lab = _dev(x_host), _dev(labels)
    sv = MT.SemanticValidation(num_classes=K, max_frames=B * T + 3, device=DEV)
    acc = R.Accumulator(K)
    bad_counts = 0
    for count, dtype in ((None, None), ([T, 1, 0][:B], torch.int32), ([T + 2, -1, 1][:B], torch.int64)):
        cnt = None if count is None else _dev(count, dtype)
        ref = acc.update(x_host, labels, count)
        got, state = _frame_counts(x, lab, cnt, B, T, K)
        np.testing.assert_array_equal(got, ref["counts"])
        assert state == [0, 0, 0, 0]
        sv.update(x, lab, cnt)
        print(hw, K, BT, count, "frame_miou", sv.last_call()[3].cpu().numpy(), ref["frame_miou"])
        _check_call(sv, ref, acc)
        bad_counts += ref["bad_count"]
    assert sv._state.cpu().tolist() == [0, bad_counts, acc.frames, 0]
    r, want = sv.results(), acc.results()
    _bits(r["miou_pc"], want["miou_pc"]), _bits(r["fscore_pc"], want["fscore_pc"]), _bits(r["cls_count"], acc.cls_count)
    assert r["miou"] == torch.from_numpy(want["miou_pc"]).mean().item() and r["binary_miou"] == float(want["binary_miou"])
    assert torch.equal(lab.cpu(), torch.from_numpy(labels))                        # the labels are never written


def test_k4096_on_7x9():
    """The largest class number: 12292 counters (48 KiB + 16 bytes) in LDS, 16 combine workgroups and the ticketed last one."""
    B, T, K, H, W = 2, 2, 4096, 7, 9
    x_host, labels = _inputs(B, T, K, H, W, seed=4096)
    x, lab = _dev(x_host), _dev(labels)
    acc = R.Accumulator(K)
    ref = acc.update(x_host, labels, [2, 1])
    cnt = _dev([2, 1], torch.int32)
    got, _ = _frame_counts(x, lab, cnt, B, T, K)
    np.testing.assert_array_equal(got, ref["counts"])
    sv = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
    sv.update(x, lab, cnt)
    _check_call(sv, ref, acc)
    sv.check()


def test_misaligned_logits_base():
    """Whole quads through the element path: a base one float past a 16-byte boundary."""
    B, T, K, H, W = 2, 2, 5, 24, 28
    x_host, labels = _inputs(B, T, K, H, W, seed=3)
    buf = torch.empty(x_host.size + 1, device=DEV)
    x = buf[1:].view(B * T, K, H, W).copy_(_dev(x_host))
    assert x.data_ptr() % 16 != 0
    acc = R.Accumulator(K)
    ref = acc.update(x_host, labels)
    got, _ = _frame_counts(x, _dev(labels), None, B, T, K)
    np.testing.assert_array_equal(got, ref["counts"])
    sv = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
    sv.update(x, _dev(labels))
    _check_call(sv, ref, acc)


def test_mask_form_and_check():
    """The uint8 mask of CAVP.predict gives the logits' result; a byte >= K sets no class counter and is counted by check()."""
    B, T, K = 2, 3, 5
    for H, W in ((24, 28), (7, 9)):
        x_host, labels = _inputs(B, T, K, H, W, seed=H)
        mask = x_host.argmax(1).astype(np.uint8)
        a = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
        b = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
        cnt = _dev([T, 2], torch.int64)
        a.update(_dev(x_host), _dev(labels), cnt)
        b.update(_dev(mask), _dev(labels), cnt)
        assert torch.equal(a._res, b._res) and torch.equal(a._last.view(torch.int32), b._last.view(torch.int32))
        b.check()
        mask[1, 0, :3] = [K, 200, 255]
        mask[5] = 77                                                               # a frame that takes no part is not read
        acc = R.Accumulator(K)
        ref = acc.update(mask, labels, [T, 2])
        assert ref["bad_mask"] == 3
        got, state = _frame_counts(_dev(mask), _dev(labels), cnt, B, T, K)
        np.testing.assert_array_equal(got, ref["counts"])
        assert state == [3, 0, 0, 0]
        c = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
        c.update(_dev(mask), _dev(labels), cnt)
        _check_call(c, ref, acc)
        with pytest.raises(CavpError, match="3 mask"):
            c.check()
        c.check()                                                                  # the counters were cleared by the raising check
        with pytest.raises(CavpError, match="1 count"):
            c.update(_dev(mask[:3]), _dev(labels[:1]), _dev([T + 1], torch.int32))
            c.check()


def test_frames_that_take_no_part_are_not_read():
    B, T, K, H, W = 3, 5, 5, 24, 28
    x_host, labels = _inputs(B, T, K, H, W, seed=5)
    count = [T, 1, 0]
    got = []
    for poison in (False, True):
        xh, lh = x_host.copy().reshape(B, T, K, H, W), labels.copy()
        if poison:
            for b in range(B):
                xh[b, count[b]:] = np.nan
                lh[b, count[b]:] = 10 ** 6
        sv = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
        sv.update(_dev(xh.reshape(B * T, K, H, W)), _dev(lh), _dev(count, torch.int32))
        sv.check()
        got.append((sv._res.cpu(), sv._last.cpu().view(torch.int32)))
    assert got[0][1][3 * K + 1 + T + 1] == torch.tensor(-1.0).view(torch.int32)   # frame (1, 1) took no part
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_nan_logits():
    """A NaN is the maximum (the first one wins); an all-NaN pixel predicts class 0."""
    B, T, K, H, W = 1, 2, 5, 7, 9
    x_host, labels = _inputs(B, T, K, H, W, seed=9)
    x_host[0, :, 0, 0] = np.nan                                                    # all NaN: class 0
    x_host[0, 3, 0, 1] = np.nan                                                    # one NaN: class 3
    x_host[1, 2:, 1, 1] = np.nan                                                   # several: the first, class 2
    labels[0, 0, 0, :2] = [0, 3]
    labels[0, 1, 1, 1] = 2
    assert R.predictions(x_host)[0, 0, :2].tolist() == [0, 3] and R.predictions(x_host)[1, 1, 1] == 2
    acc = R.Accumulator(K)
    ref = acc.update(x_host, labels)
    got, _ = _frame_counts(_dev(x_host), _dev(labels), None, B, T, K)
    np.testing.assert_array_equal(got, ref["counts"])
    sv = MT.SemanticValidation(num_classes=K, max_frames=2, device=DEV)
    sv.update(_dev(x_host), _dev(labels))
    _check_call(sv, ref, acc)


def test_frame_without_a_hit_scores_nan():
    """No class with a non-zero IoU: frame_miou is 0 / 0, the reference's NaN, and the frame still counts its classes as seen."""
    B, T, K, H, W = 1, 2, 3, 7, 9
    x_host, labels = _inputs(B, T, K, H, W, seed=11)
    labels[0, 1] = (x_host[1].argmax(0) + 1) % K                                   # never the prediction
    acc = R.Accumulator(K)
    ref = acc.update(x_host, labels)
    assert np.isnan(ref["frame_miou"][1]) and not np.isnan(ref["frame_miou"][0]) and ref["cls_count"].min() >= 1
    sv = MT.SemanticValidation(num_classes=K, max_frames=2, device=DEV)
    sv.update(_dev(x_host), _dev(labels))
    _check_call(sv, ref, acc)
    assert bool(torch.isnan(sv.last_call()[3][1])) and not bool(torch.isnan(sv.accumulators()).any())


# ---- the reference's numbers -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


CASES = {"vec": 5, "sca": 3}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("split", [False, True])
def test_fixture(z, name, split):
    K = CASES[name]
    logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
    B, T = labels.shape[:2]
    x, lab = _dev(logits), _dev(labels)
    sv = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
    if split:
        for b, run in enumerate(("a", "b")):
            sv.update(x[b], lab[b])
            ious, fscores, cls_count, frame_miou = (t.cpu().numpy() for t in sv.last_call())
            _bits(ious, z[f"{name}_{run}_ious"]), _bits(fscores, z[f"{name}_{run}_fscores"]), _bits(cls_count, z[f"{name}_{run}_cls_count"])
            _ulp(frame_miou, z[f"{name}_{run}_vid"])
        want = [z[f"{name}_two_{k}"] for k in ("ious", "fscores", "cls_count")]
    else:
        sv.update(x.flatten(0, 1), lab, _dev([T] * B, torch.int64))
        frame_miou = sv.last_call()[3].cpu().numpy()
        print(name, "frame_miou", frame_miou, z[f"{name}_one_vid"])
        _ulp(frame_miou, z[f"{name}_one_vid"])
        _ulp(sv._last[3 * K].cpu().numpy() / np.float32(B * T), z[f"{name}_one_binary"])
        want = [z[f"{name}_one_{k}"] for k in ("ious", "fscores", "cls_count")]
    _bits(sv.accumulators(), np.stack(want))
    assert sv.frames() == B * T and int(sv._scratch.ne(0).sum()) == 0
    sv.check()


@pytest.mark.parametrize("name", list(CASES))
def test_drop_in_functions(z, name):
    logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
    x, lab = _dev(logits).flatten(0, 1), _dev(labels).flatten(0, 1)
    ious, fscores, cls_count, vid = MT.calc_color_miou_fscore(x, lab, T=3)
    assert isinstance(vid, list) and len(vid) == 6 and all(v.dim() == 0 and v.dtype == torch.float32 for v in vid)
    assert all(t.dtype == torch.float32 and not t.is_cuda for t in (ious, fscores, cls_count))
    _bits(ious, z[f"{name}_one_ious"]), _bits(fscores, z[f"{name}_one_fscores"]), _bits(cls_count, z[f"{name}_one_cls_count"])
    _ulp(torch.stack(vid).numpy(), z[f"{name}_one_vid"])
    ious2, cls2 = MT.calc_color_miou(x, lab, T=3)
    _bits(ious2, z[f"{name}_one_ious2"]), _bits(cls2, z[f"{name}_one_cls2"])
    b = MT.calc_binary_miou(x, lab)
    assert b.dim() == 0 and b.dtype == torch.float32
    _ulp(b.numpy(), z[f"{name}_one_binary"])
    ious_a, _, _, vid_a = MT.calc_color_miou_fscore(x[:3], lab[:3].float())      # the reference takes any label dtype
    _bits(ious_a, z[f"{name}_a_ious"])
    assert len(vid_a) == 3


# ---- update_lowres ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw", [(24, 28), (7, 9)])
def test_update_lowres_equals_update_on_the_upsample(hw, dtype):
    B, T, K = 2, 3, 5
    (H, W), N = hw, 6
    g = torch.Generator().manual_seed(H)
    lo = (torch.randn((N, (H + 3) // 4, (W + 3) // 4, K), generator=g) * 2).to(dtype).to(DEV)
    full = ops.bilinear_to_nchw(lo, torch.empty((N, K, H, W), dtype=torch.float32, device=DEV), False)
    _, lab_host = _inputs(B, T, K, H, W, seed=2)
    labels = torch.where(_dev(np.random.RandomState(1).rand(B, T, H, W)) < 0.6, full.argmax(1).view(B, T, H, W), _dev(lab_host))
    count = _dev([T, 2], torch.int32)
    a = MT.SemanticValidation(num_classes=K, max_frames=N, device=DEV)
    b = MT.SemanticValidation(num_classes=K, max_frames=N, device=DEV)
    for _ in range(2):
        a.update(full, labels, count)
        b.update_lowres(lo, labels, count, input_shape=(H, W))
    assert torch.equal(a._res, b._res) and torch.equal(a._last.view(torch.int32), b._last.view(torch.int32))
    assert a.frames() == 10 and float(a.accumulators()[0].sum()) > 0
    assert int(b._scratch.ne(0).sum()) == 0


# ---- reset, capture --------------------------------------------------------------------------------------------------------------
def test_reset():
    B, T, K, H, W = 2, 3, 5, 7, 9
    x_host, labels = _inputs(B, T, K, H, W, seed=31)
    x, lab = _dev(x_host), _dev(labels)
    sv = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
    sv.update(x, lab)
    first = sv._res.clone()
    sv.update(x, lab)
    assert sv.frames() == 2 * B * T and not torch.equal(sv._res, first)
    sv.reset()
    assert sv.frames() == 0 and float(sv.accumulators().abs().sum()) == 0 and float(sv._acc.abs().sum()) == 0
    with pytest.raises(CavpError, match="no frame"):
        sv.results()
    sv.update(x, lab)
    assert torch.equal(sv._res, first)
    sv.check()


def test_update_captured_in_a_graph():
    from cavp_amd.train import _no_gc_during_capture
    B, T, K, H, W = 3, 5, 5, 24, 28
    data = [_inputs(B, T, K, H, W, seed=41 + i) for i in range(2)]
    xs, labs = [_dev(d[0]) for d in data], [_dev(d[1]) for d in data]
    cnts = [_dev([T, 0, 3], torch.int32), _dev([2, T, 1], torch.int32)]

    eager = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
    for i in range(2):
        eager.update(xs[i], labs[i], cnts[i])
    assert eager.frames() == 16

    sv = MT.SemanticValidation(num_classes=K, max_frames=B * T, device=DEV)
    x, lab, cnt = xs[0].clone(), labs[0].clone(), cnts[0].clone()                  # the static buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sv.update(x, lab, cnt)             # the first call allocates: it cannot be the captured one
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        sv.update(x, lab, cnt)
    sv.reset()
    assert sv.frames() == 0
    for i in range(2):
        x.copy_(xs[i]), lab.copy_(labs[i]), cnt.copy_(cnts[i])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sv._res, eager._res) and torch.equal(sv._last.view(torch.int32), eager._last.view(torch.int32))
    assert int(sv._scratch.ne(0).sum()) == 0
    sv.check()
