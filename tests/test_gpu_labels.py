"""The device label stage (cavp_amd/labels.py, csrc/labels.hip) against the numpy restatement of its specification
(tests/_labels_ref.py, held to the reference's torch expressions by tests/test_labels_host.py).  Everything it produces is an
integer: every comparison is exact equality.  B = 3 with 5 x 7 images (35 pixels: no 16-byte alignment of the second image, the
element-load kernels) and 32 x 48 (the 16-byte-load kernels, int64 and uint8)."""
import numpy as np
import pytest
import torch

from tests import _labels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(5, 7), (32, 48)]


def _stage(K, **kw):
    from cavp_amd.labels import LabelStage
    kw.setdefault("max_batch", 8)
    return LabelStage(num_classes=K, device=DEV, **kw)


def _labels(rng, K, hw, B=3):
    """Patches of a few classes of [0, K) and 255; image 1 is 255 only; the largest class sits in the last pixel of the last image
    and nowhere else."""
    H, W = hw
    top = K - 1 if K - 1 != 255 else 254
    pool = np.array(sorted({0, 1 % K, (K // 2), max(top - 1, 0), 255} - {top}), dtype=np.int64)
    lab = np.repeat(rng.choice(pool, size=(B, H, (W + 2) // 3)), 3, axis=2)[:, :, :W]
    lab = np.ascontiguousarray(lab)
    lab[1] = 255
    lab[B - 1, H - 1, W - 1] = top
    return lab, top


def _run(st, lab, dtype):
    t = torch.from_numpy(lab.astype(np.uint8) if dtype == torch.uint8 else lab).to(DEV)
    keep = t.clone()
    out = st(t)
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "the input was modified"
    return out, t


def _assert_equals_ref(out, exp):
    assert out.img_label.dtype == torch.int64 and out.label.dtype == torch.int64
    assert np.array_equal(out.img_label.cpu().numpy(), exp["img_label"])
    assert np.array_equal(out.label.cpu().numpy(), exp["label"])


@pytest.mark.parametrize("K", [2, 71, 256])
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("hw", SHAPES, ids=["5x7", "32x48"])
def test_multi_hot(hw, dtype, K):
    rng = np.random.default_rng(K + hw[0])
    lab, top = _labels(rng, K, hw)
    st = _stage(K)
    exp = R.label_stage(lab, K)
    assert exp["bad"] == 0 and not exp["img_label"][1].any() and exp["img_label"][2, top] == 1 and exp["img_label"][:2, top].sum() == 0
    for _ in range(2):                                   # the second call finds the masks cleared by the first
        out, t = _run(st, lab, dtype)
        _assert_equals_ref(out, exp)
        st.check()
    if dtype == torch.int64:
        assert out.label.data_ptr() == t.data_ptr()      # nothing changes the label: the input itself


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("hw", SHAPES, ids=["5x7", "32x48"])
def test_out_of_range_value_is_counted_and_nothing_is_written_outside(hw, dtype):
    """200 with K = 71 (and, for int64, -3 and 2^40): counted, no class bit, and the bytes around img_label and label - carved out
    of sentinel-filled buffers - are untouched."""
    from cavp_amd._lib import CavpError
    from cavp_amd.labels import LabelResult
    K, B = 71, 3
    rng = np.random.default_rng(7)
    lab, _ = _labels(rng, K, hw)
    lab[0, 0, :3] = 200
    n_bad = 3
    if dtype == torch.int64:
        lab[2, 1, 0], lab[2, 2, 1] = -3, 1 << 40
        n_bad = 5
    st = _stage(K, binary=True)
    exp = R.label_stage(lab, K, binary=True)
    assert exp["bad"] == n_bad
    guard = 64
    n_img, n_lab = B * K, B * hw[0] * hw[1]
    buf_img = torch.full((n_img + 2 * guard,), -77, dtype=torch.int64, device=DEV)
    buf_lab = torch.full((n_lab + 2 * guard,), -77, dtype=torch.int64, device=DEV)
    out = LabelResult(B, K, hw, torch.device(DEV), True)
    out.img_label = buf_img[guard:guard + n_img].view(B, K)
    out.label = buf_lab[guard:guard + n_lab].view(B, *hw)
    t = torch.from_numpy(lab.astype(np.uint8) if dtype == torch.uint8 else lab).to(DEV)
    st(t, out=out)
    torch.cuda.synchronize()
    _assert_equals_ref(out, exp)
    for buf, n in ((buf_img, n_img), (buf_lab, n_lab)):
        assert (buf[:guard] == -77).all() and (buf[guard + n:] == -77).all()
    with pytest.raises(CavpError, match=f"{n_bad} pixel"):
        st.check()
    st.check()               # the counter was cleared by the report


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("hw", SHAPES, ids=["5x7", "32x48"])
@pytest.mark.parametrize("binary", [False, True])
def test_chained_remap(hw, dtype, binary):
    """remap[3] = 5 with 5 present in image 0 (moved on to 9) and absent in image 2 (stays 5); a self-map, a map downwards onto a
    value whose step is over, a map onto 255, and a -1 entry on a raw value and at the end of a chain."""
    from cavp_amd._lib import CavpError
    K = 24
    remap = np.full(256, -1, dtype=np.int32)
    remap[[3, 5, 7, 8, 10, 20, 21, 30]] = [5, 9, 7, 2, 255, 21, -1, -1]
    remap[2] = 1
    rng = np.random.default_rng(11)
    H, W = hw
    lab = np.repeat(rng.choice(np.array([0, 2, 3, 5, 7, 8, 10, 255]), size=(3, H, (W + 1) // 2)), 2, axis=2)[:, :, :W].astype(np.int64)
    lab = np.ascontiguousarray(lab)
    lab[2][lab[2] == 5] = 0
    lab[2, 0, :2] = 3
    lab[0, 1, 0], lab[0, 1, 1] = 5, 3
    lab[1, 0, 0], lab[1, 0, 1] = 20, 30                 # 21 absent: 20 ends at 21, a class; 30 -> -1: bad
    lab[0, 2, 0], lab[0, H - 1, W - 1] = 20, 21         # 21 present: 20 moves on to 21, whose entry is -1: both pixels bad, kept 21
    exp = R.label_stage(lab, K, remap=remap, binary=binary)
    assert exp["bad"] == 3 and exp["img_label"][0, 21] == 1 and exp["img_label"][1, 21] == 1
    assert (exp["label"][0][lab[0] == 3] == (1 if binary else 9)).all() and (exp["label"][2][lab[2] == 3] == (1 if binary else 5)).all()
    assert exp["img_label"][0, 9] == 1 and exp["img_label"][0, 5] == 0 and exp["img_label"][2, 5] == 1
    st = _stage(K, remap=remap, binary=binary)
    for _ in range(2):
        out, _t = _run(st, lab, dtype)
        _assert_equals_ref(out, exp)
        with pytest.raises(CavpError, match="3 pixel"):
            st.check()


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("hw", SHAPES, ids=["5x7", "32x48"])
def test_any_foreground(hw, dtype):
    """All zero -> [1, 0]; a single 255 pixel -> [0, 1] (non-zero in the reference's sum); a single 1 in the last pixel -> [0, 1]."""
    lab = np.zeros((3,) + hw, dtype=np.int64)
    lab[1, 2, 3] = 255
    lab[2, -1, -1] = 1
    st = _stage(2, mode="any_foreground")
    exp = R.label_stage(lab, 2, "any_foreground")
    assert exp["img_label"].tolist() == [[1, 0], [0, 1], [0, 1]]
    out, _t = _run(st, lab, dtype)
    _assert_equals_ref(out, exp)
    st.check()
    out, _t = _run(_stage(2, mode="any_foreground", binary=True), lab, dtype)
    _assert_equals_ref(out, R.label_stage(lab, 2, "any_foreground", binary=True))


def test_random_tables_against_the_loop():
    """Twenty random remap tables over raw values 1 .. 40 into [0, 16) and up, 3 x 32 x 48 uint8: the device's per-value closed form
    equals the literal loop."""
    rng = np.random.default_rng(3)
    K = 48
    for trial in range(20):
        remap = np.full(256, -1, dtype=np.int32)
        remap[1:41] = rng.integers(0, 48, 40)
        lab = np.repeat(rng.integers(0, 41, size=(3, 32, 12)), 4, axis=2).astype(np.int64)
        lab[rng.random(lab.shape) < 0.05] = 255
        exp = R.label_stage(lab, K, remap=remap)
        st = _stage(K, remap=remap)
        out, _t = _run(st, lab, torch.uint8)
        _assert_equals_ref(out, exp)
        st.check()


def test_graph_capture_chain_augment_labels_pairs():
    """FrameAugment(resize=True) -> LabelStage(remap) -> PairBuilder captured in one torch.cuda.graph on one stream (capture raises
    if anything synchronises): three replays with fresh staged inputs equal the eager chain run after the same manual_seed reset, and img_label
    equals the restatement applied to the label the graph produced."""
    from cavp_amd.augment import AugResult, FrameAugment
    from cavp_amd.labels import LabelResult
    from cavp_amd.pairs import PairBuilder
    B, K, S, A, crop, stage, seed = 4, 6, 2, 64, (24, 40), (48, 64), 5
    remap = np.full(256, -1, dtype=np.int32)
    remap[[11, 12, 13, 3]] = [1, 3, 2, 4]               # 12 -> 3 with raw 3 present: on to 4

    def make():
        aug = FrameAugment(crop=crop, scales=(0.75, 1.0, 1.25), jitter=None, seed=seed, device=DEV, max_batch=B, stage=stage, resize=True)
        return aug, _stage(K, remap=remap, max_batch=B), PairBuilder(num_classes=K, bank_slots=S, wave_len=A, ow_rate=0.5, seed=seed,
                                                                     device=DEV, max_batch=B)

    def staged(k):
        rng = np.random.default_rng(100 + k)
        frames = rng.integers(0, 256, (B,) + stage + (3,), dtype=np.uint8)
        masks = np.zeros((B,) + stage, dtype=np.uint8)
        for b in range(B):
            for v in rng.choice([11, 12, 13, 3], size=2, replace=False):
                y, x = rng.integers(0, 30), rng.integers(0, 40)
                masks[b, y:y + 18, x:x + 24] = v
        masks[:, :2] = 255
        wav = rng.standard_normal((B, 1, A)).astype(np.float32)
        sizes = np.tile(np.asarray(stage, dtype=np.int32), (B, 1))
        return [torch.from_numpy(a).to(DEV) for a in (frames, masks, sizes, wav)]

    def chain(objs, ins, outs=(None, None, None)):
        aug, st, pb = objs
        a = aug(ins[0], ins[1], ins[2], out=outs[0])
        lab = st(a.label, out=outs[1])
        return a, lab, pb(ins[3], lab.label, lab.img_label, True, out=outs[2])

    cap, eager = make(), make()
    ins = staged(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = chain(cap, ins)                           # warm-up: allocates the device state and the out= buffers
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for objs in (cap, eager):
        objs[0].manual_seed(seed)
        objs[2].manual_seed(seed)
    chain(eager, ins)                                    # the same history for the eager bank as the warm-up gave the captured one
    eager[0].manual_seed(seed)
    eager[2].manual_seed(seed)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(cap, ins, outs)
    seen = 0
    for k in range(3):
        for dst, src in zip(ins, staged(k + 1)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        a, lab, pr = chain(eager, ins)
        assert torch.equal(outs[0].image, a.image) and torch.equal(outs[0].label, a.label), k
        assert torch.equal(outs[1].img_label, lab.img_label) and torch.equal(outs[1].label, lab.label), k
        for f in ("waveforms", "label_shuffle", "if_match", "img_label_shuffle", "perm", "source"):
            assert torch.equal(getattr(outs[2], f), getattr(pr, f)), (k, f)
        exp = R.label_stage(outs[0].label.cpu().numpy(), K, remap=remap)
        assert np.array_equal(outs[1].img_label.cpu().numpy(), exp["img_label"]) and exp["bad"] == 0
        assert np.array_equal(outs[1].label.cpu().numpy(), exp["label"])
        seen += int(exp["img_label"][:, 1:].sum())
        cap[1].check()
        cap[0].check()
        cap[2].last_plan()
    assert seen > 0
