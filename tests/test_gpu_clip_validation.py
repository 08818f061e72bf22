"""GPU checks of cavp_amd.metrics.ClipValidation (csrc/metrics.hip: cavp_clipval_frame_counts, cavp_clipval_combine) against the
reference's own numbers (tests/golden/clip_validation.npz) and the CPU restatement tests/_clipval_ref.py.  Everything compared is
an integer, or a float finalised from equal integers by the same expressions: exact equality throughout."""
import os
import types

import numpy as np
import pytest
import torch

from cavp_amd import metrics as MT
from cavp_amd._lib import CavpError
from tests import _clipval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_validation.npz")


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a, dtype=dtype).to(DEV)


def _assert_equals_ref(cv, ref):
    np.testing.assert_array_equal(cv.counts().cpu().numpy(), ref["counts"])
    assert cv.frames() == ref["frames"]
    assert cv._state.cpu().tolist()[:3] == ref["bad"]
    assert int(cv._hist.ne(0).sum()) == 0 and int(cv._conf.ne(0).sum()) == 0      # the scratch is zero at rest


# ---- the reference's numbers -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("form", ["logits", "mask"])
@pytest.mark.parametrize("split", [False, True])
def test_fixture(z, name, form, split):
    lq, labels, mask_num = z[f"{name}_logits_q"], z[f"{name}_labels"], z[f"{name}_mask_num"]
    B, T, K = lq.shape[0], lq.shape[1], lq.shape[2]
    logits = torch.from_numpy(lq.astype(np.float32) / 8)
    pred = (logits if form == "logits" else logits.argmax(2).to(torch.uint8)).to(DEV)
    lab, cnt = _dev(labels), _dev(mask_num, torch.int32)
    cv = MT.ClipValidation(num_classes=K, max_frames=B * T, device=DEV)
    parts = [slice(0, 1), slice(1, B)] if split and B > 1 else [slice(0, B)]
    for s in parts:
        cv.update(pred[s].flatten(0, 1), lab[s], cnt[s])
    np.testing.assert_array_equal(cv.counts().cpu().numpy(), z[f"{name}_M"])
    assert cv.frames() == tuple(z[f"{name}_frames"])
    res = cv.results()
    assert [float(v) for v in res[0] + res[1]] == z[f"{name}_results"].tolist()
    perf = MT.get_performance(cv.all_miou, cv.all_fg) + MT.get_performance(cv.ms_miou, cv.ms_fg)
    assert [float(v) for v in perf] == z[f"{name}_results"].tolist()
    assert cv.all_miou.counts().data_ptr() == cv.counts()[0].data_ptr()             # the accessors read, they do not copy
    assert torch.equal(lab.cpu(), torch.from_numpy(labels))                         # the labels are never written
    cv.check()


# ---- sweep against the restatement -----------------------------------------------------------------------------------------------
def _spec(kind, hw, K, rs):
    """{value: pixels} of one label frame; kinds as in tools/make_golden_clipval.py, sized for 320 / 323 pixels."""
    top = min(K, 22) - 1
    specs = [
        {0: 110, 1: 105, top: hw - 215},                       # three qualifying values
        {0: 160, 1: hw - 160},                                 # two
        {0: hw - 201, 1: 100, top: 101},                       # exactly 100 does not qualify, 101 does
        {0: 110, 1: 105, 255: hw - 215},                       # the ignore value is the third one
        {0: 105, top: 101, K: 57, K + 1: hw - 263},            # K and K + 1 are values of their own
        {0: 110, top: 105, 255: 55, -1: hw - 270},             # -1 and 255 are one value
    ]
    if kind < len(specs):
        return specs[kind]
    vals = rs.choice(np.r_[0:K, -1, 255, K, K + 1], size=hw)   # anything
    return {int(v): int(n) for v, n in zip(*np.unique(vals, return_counts=True))}


def _labels(B, T, H, W, K, seed):
    rs = np.random.RandomState(seed)
    out = np.empty((B, T, H * W), dtype=np.int64)
    for i in range(B * T):
        spec = _spec((i + seed) % 7, H * W, K, rs)
        flat = np.concatenate([np.full(n, v, dtype=np.int64) for v, n in spec.items()])
        assert flat.size == H * W
        out[i // T, i % T] = rs.permutation(flat)
    return out.reshape(B, T, H, W)


def _logits(N, C, H, W, seed, misalign):
    """Quantised logits (exact ties); misalign: a dense view one float past a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (N * C * H * W + 1,), generator=g).float().div_(8).to(DEV)
    v = (x[1:] if misalign else x[:-1]).view(N, C, H, W)
    assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == misalign
    return v


@pytest.mark.parametrize("K", [3, 71, 127, 128])
@pytest.mark.parametrize("BT", [(1, 1), (3, 5)])
@pytest.mark.parametrize("hw", [(16, 20), (17, 19)])
def test_sweep(hw, BT, K):
    (H, W), (B, T) = hw, BT
    C = min(K, 22)
    labels = _labels(B, T, H, W, K, seed=K + B)
    logits = _logits(B * T, C, H, W, seed=K, misalign=(H * W) % 4 != 0)
    mask = logits.argmax(1).to(torch.uint8)
    lab = _dev(labels)
    counts = [[1], [0]] if B == 1 else [[T, 0, 2], [1, T, T - 1]]
    runs = [(logits, counts[0], torch.int32), (mask, counts[0], torch.int64), (mask, counts[1], torch.int32),
            (logits, counts[1], torch.int64), (mask, None, None)]
    if (H * W) % 4 == 0:   # whole quads, but the mask starts one byte past a 4-byte boundary: the element path of the mask input
        shifted = torch.empty(mask.numel() + 1, dtype=torch.uint8, device=DEV)[1:].view_as(mask).copy_(mask)
        assert shifted.is_contiguous() and shifted.data_ptr() % 4 == 1
        runs.append((shifted, None, None))
    for pred, count, dtype in runs:
        ref = R.clip_validation(pred.cpu(), labels, count, K)
        cv = MT.ClipValidation(num_classes=K, max_frames=B * T, device=DEV)
        cv.update(pred, lab, None if count is None else _dev(count, dtype))
        _assert_equals_ref(cv, ref)
    assert ref["frames"][0] == B * T


def test_several_workgroups_per_frame():
    """64 x 64: two workgroups share a frame's scratch; dense [N, H, W] labels without a count."""
    K, N, H, W = 71, 3, 64, 64
    rs = np.random.RandomState(5)
    labels = rs.choice(np.r_[0:6, 255, -1, K], size=(1, N, H, W), p=[.3, .2, .2, .1, .05, .05, .04, .03, .03]).astype(np.int64)
    labels[0, 1] = np.where((labels[0, 1] > 1) | (labels[0, 1] < 0), 0, labels[0, 1])     # a frame with two values only
    logits = _logits(N, 22, H, W, seed=9, misalign=False)
    for pred in (logits, logits.argmax(1).to(torch.uint8)):
        ref = R.clip_validation(pred.cpu(), labels, None, K)
        cv = MT.ClipValidation(num_classes=K, max_frames=N, device=DEV)
        cv.update(pred, _dev(labels[0]))
        _assert_equals_ref(cv, ref)
    assert ref["frames"] == (3, 2)


def test_one_pixel_flips_membership():
    """The largest class value has 101 pixels: the frame is multi-source; with one of them relabelled it is not."""
    K, H, W = 3, 16, 20
    flat = np.concatenate([np.full(n, v, dtype=np.int64) for v, n in {0: 110, 1: 109, 2: 101}.items()])
    labels = np.random.RandomState(3).permutation(flat).reshape(1, 1, H, W)
    mask = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    got = []
    for flip in (False, True):
        lab = labels.copy()
        if flip:
            y, x = np.argwhere(lab[0, 0] == 2)[0]
            lab[0, 0, y, x] = 0
        cv = MT.ClipValidation(num_classes=K, max_frames=1, device=DEV)
        cv.update(mask, _dev(lab))
        assert cv.frames() == R.clip_validation(mask.cpu(), lab, None, K)["frames"]
        got.append(cv.frames())
    assert got == [(1, 1), (1, 0)]


# ---- input handling --------------------------------------------------------------------------------------------------------------
def _banded(numel, dtype, sentinel, pad=64):
    """A zeroed buffer of `numel` elements between two sentinel-filled bands: (whole, middle view)."""
    whole = torch.full((numel + 2 * pad,), sentinel, dtype=dtype, device=DEV)
    whole[pad:pad + numel] = 0
    return whole, whole[pad:pad + numel]


def test_guards():
    """Mask bytes >= K, labels >= 256 and counts outside [0, T] are counted and dropped; nothing is written outside the buffers."""
    K, B, T, H, W = 3, 3, 2, 16, 20
    labels = _labels(B, T, H, W, K, seed=11)
    labels[0, 0, 0, :5] = 300
    labels[0, 1, 3, 3] = 256
    labels[2, 0, 1, 1] = 2 ** 40
    g = torch.Generator().manual_seed(2)
    mask = torch.randint(0, K, (B * T, H, W), generator=g).to(torch.uint8)
    mask[0, 0, :7] = 255                   # five of them under a label of 300
    mask[1, 5, 5] = K
    mask[4, 2, 2] = 200
    count = [T + 2, -1, 1]
    ref = R.clip_validation(mask, labels, count, K)
    assert ref["bad"] == [7, 2 + 1 + 1, 2] and ref["frames"][0] == 3

    cv = MT.ClipValidation(num_classes=K, max_frames=B * T, device=DEV)
    bands = [_banded(B * T * 256, torch.int32, -1), _banded(B * T * cv.nbins, torch.int32, -1), _banded(B * T, torch.int32, -1),
             _banded(2 * cv.nbins, torch.int64, -7), _banded(2, torch.int64, -7), _banded(4, torch.int64, -7)]
    cv._bind(*(mid for _, mid in bands))
    lab = _dev(labels)
    for dtype in (torch.int32, torch.int64):
        cv.reset()
        cv._state.zero_()
        cv.update(mask.to(DEV), lab, _dev(count, dtype))
        _assert_equals_ref(cv, ref)
        for (whole, mid), sentinel in zip(bands, (-1, -1, -1, -7, -7, -7)):
            assert int((whole != sentinel).sum()) <= mid.numel() and bool((whole[:64] == sentinel).all()) \
                and bool((whole[-64:] == sentinel).all())
        with pytest.raises(CavpError, match="7 label"):
            cv.check()
        cv.check()                          # the counters were cleared by the raising check


def test_logits_wider_than_classes_raise():
    cv = MT.ClipValidation(num_classes=3, max_frames=2, device=DEV)
    with pytest.raises(CavpError):
        cv.update(torch.zeros((2, 4, 8, 8), device=DEV), torch.zeros((2, 8, 8), dtype=torch.int64, device=DEV))
    with pytest.raises(CavpError):
        cv.update(torch.zeros((2, 8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.int64, device=DEV))


# ---- no sync: graph capture ------------------------------------------------------------------------------------------------------
def test_update_captured_in_a_graph():
    from cavp_amd.train import _no_gc_during_capture
    K, B, T, H, W = 22, 3, 5, 16, 20
    labels = _labels(B, T, H, W, K, seed=4)
    lab, cnt = _dev(labels), _dev([T, 0, 3], torch.int32)
    mask = _logits(B * T, K, H, W, seed=1, misalign=False).argmax(1).to(torch.uint8)
    ref = R.clip_validation(mask.cpu(), labels, [T, 0, 3], K)

    eager = MT.ClipValidation(num_classes=K, max_frames=B * T, device=DEV)
    eager.update(mask, lab, cnt)
    _assert_equals_ref(eager, ref)
    once, once_frames = eager.counts().clone(), eager.frames()
    assert int(once[1].sum()) > 0

    cv = MT.ClipValidation(num_classes=K, max_frames=B * T, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cv.update(mask, lab, cnt)          # the first call allocates: it cannot be the captured one
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
        cv.update(mask, lab, cnt)
    cv.reset()
    assert int(cv.counts().ne(0).sum()) == 0 and cv.frames() == (0, 0)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cv.counts(), 2 * once)
    assert cv.frames() == (2 * once_frames[0], 2 * once_frames[1])
    assert int(cv._hist.ne(0).sum()) == 0 and int(cv._conf.ne(0).sum()) == 0
    cv.check()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_predict_and_update_equal_the_frame_loop():
    """Two clips of three frames through CAVP.predict + one update, against the reference-shaped loop: one frame per forward,
    MIoU / ForegroundDetect on its logits, the predicate by torch.unique on the host."""
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_inputs, synth_state_dict
    from tests._golden_util import load_case
    K, B, T, H, W = 22, 2, 3, 96, 96
    N = B * T
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=load_case("c1p_eval")[1]["lds"],
                                 audio_backbone="vgg", num_classes=K, batch_size=N, local_rank="cpu")
    m = CAVP(50, None, num_classes=K, args=args)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.eval().to(DEV).set_compute_dtype(torch.float32)
    image, audio, _ = synth_inputs(N, (H, W), num_classes=K, seed=0)
    image, audio = image.to(DEV), audio.to(DEV)
    # label frames: quadrants and stripes, so that some frames have three values above 100 pixels and some have two
    labels = torch.zeros((B, T, H, W), dtype=torch.int64)
    labels[0, 0, :48, :48], labels[0, 0, 48:, 48:] = 3, 7                        # 0, 3, 7: multi-source
    labels[0, 1, :, :40] = 5                                                     # 0, 5: not
    labels[0, 2, :10, :10], labels[0, 2, 50:, :] = 9, 255                        # 0, 255 and 9 at exactly 100 pixels: not
    labels[1, 0, :10, :10], labels[1, 0, 10, 0], labels[1, 0, 50:, :] = 9, 9, 255   # ... at 101: multi-source
    labels[1, 1, :30], labels[1, 1, 30:60] = 21, 22                              # 21, 22 (>= K), 0: multi-source
    labels[1, 2] = 4                                                             # beyond count: never read
    count = [T, 2]
    lab = labels.to(DEV)

    cv = MT.ClipValidation(num_classes=K, max_frames=N, device=DEV)
    cv.update(m.predict(image, audio), lab, _dev(count, torch.int64))

    loop = [MT.MIoU(K, 255, 0), MT.ForegroundDetect(K), MT.MIoU(K, 255, 0), MT.ForegroundDetect(K)]
    frames = [0, 0]
    for b in range(B):
        for t in range(count[b]):
            i = b * T + t
            with torch.no_grad():
                out = m(image[i:i + 1], audio[i:i + 1], eval_mode=True)[0]
            y = lab[b, t][None]
            loop[0].update(out, y)
            loop[1].update(out, y)
            frames[0] += 1
            uniq_id, cnt = torch.where(y == 255, -1, y).unique(return_counts=True)
            if uniq_id[cnt > 100].shape[0] > 2:
                loop[2].update(out, y)
                loop[3].update(out, y)
                frames[1] += 1
    assert frames == [5, 3] and cv.frames() == tuple(frames)
    assert torch.equal(cv.counts()[0], loop[0].counts()) and torch.equal(cv.counts()[0], loop[1].counts())
    assert torch.equal(cv.counts()[1], loop[2].counts()) and torch.equal(cv.counts()[1], loop[3].counts())
    res = cv.results()
    want = MT.get_performance(loop[0], loop[1]) + MT.get_performance(loop[2], loop[3])
    assert [float(v) for v in res[0] + res[1]] == [float(v) for v in want]
    cv.check()
