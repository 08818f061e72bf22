"""The device store (cavp_amd/store.py, csrc/store.hip) against the numpy restatement tests/_store_ref.py.  Every comparison is
bit-exact.  The restatement writes INTO copies of the buffers as they were before the feed (0xA5 everywhere), so whole-buffer
equality holds the windows to the items AND everything outside them to "not written"."""
import numpy as np
import pytest
import torch

from tests import _store_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("frames", "masks", "sizes", "pcm", "length", "rate_idx", "n_ch", "index")
NP = {torch.int16: np.int16, torch.float32: np.float32}


def _make(items, stage, S, Cm, Lmax, dtype):
    from cavp_amd.store import DeviceStore
    st = DeviceStore(stage=stage, max_sources=S, max_channels=Cm, max_len=Lmax, pcm_dtype=dtype, device=DEV)
    for it in items:
        st.append(*it)
    return st.freeze()


def _item(rng, h, w, srcs, dtype):
    """srcs: [(n_ch, len, rate_idx)]"""
    if dtype is np.int16:
        pcm = [(rng.integers(-32768, 32768, (c, n)).astype(np.int16), r) for c, n, r in srcs]
    else:
        pcm = [(rng.standard_normal((c, n)).astype(np.float32), r) for c, n, r in srcs]
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8), pcm


def _sentinel(res):
    """0xA5 into every byte of every output, the tables included."""
    for name in FIELDS:
        getattr(res, name).view(-1).view(torch.uint8).fill_(0xA5)


def _host(res):
    return {name: getattr(res, name).cpu().numpy() for name in FIELDS}


def _feed_and_compare(feeder, ref, res, index=None, what=""):
    _sentinel(res)
    want = ref.feed(_host(res), index=None if index is None else np.asarray(index))
    feeder.feed(out=res, index=None if index is None else torch.tensor(index, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    got = _host(res)
    for name in FIELDS:
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), f"{what}: {name}"
    return got


def _small_items(dtype, rng):
    """N = 7 on a 12 x 20 stage: 1 x 1, the whole slot, 21-byte rows, w = 16; source counts 0, 1, 2, odd lengths, 1 and 2 channels."""
    spec = [(1, 1, []), (12, 20, [(2, 50, 1)]), (5, 7, [(1, 33, 0), (2, 7, 2)]), (3, 16, [(2, 1, 0)]), (12, 3, []),
            (7, 20, [(1, 49, 3), (1, 50, 0)]), (2, 19, [(2, 15, 1)])]
    return [_item(rng, h, w, s, dtype) for h, w, s in spec]


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_gather_equals_the_restatement(dtype):
    """B = 3 over two epochs of N = 7 (spe = 2): windows, tables and the untouched rest, for both PCM types; item(i) reads back
    what was appended; nbytes is the packed size."""
    from cavp_amd.store import BatchFeeder, FeedResult
    items = _small_items(NP[dtype], np.random.default_rng(0))
    st = _make(items, (12, 20), 2, 2, 50, dtype)
    assert len(st) == 7 and st.arena_bytes()["frames"] == sum(f.size for f, _, _ in items)
    assert st.nbytes == sum(st.arena_bytes().values()) + 7 * (8 + 8 + 8 + 4) + 7 * 2 * (8 + 4 + 4 + 4)
    for i, (f, m, p) in enumerate(items):
        gf, gm, gp = st.item(i)
        assert np.array_equal(gf, f) and np.array_equal(gm, m)
        assert all(np.array_equal(a, b) and ra == rb for (a, ra), (b, rb) in zip(gp, p)) and len(gp) == len(p)
    fd, ref = BatchFeeder(st, batch=3, seed=5), R.StoreRef(items, B=3, seed=5)
    res = FeedResult(3, st, DEV)
    seen = set()
    for t in range(4):
        got = _feed_and_compare(fd, ref, res, what=f"step {t}")
        seen |= set(got["index"].tolist())
    assert len(seen) >= 6 and fd.step() == 4
    # every item once more through index=, so that each special size is gathered whatever the draws were
    for idx in ([0, 1, 2], [3, 4, 5], [6, 1, 1]):
        _feed_and_compare(fd, ref, res, index=idx, what=f"index {idx}")
    fd.check()


def test_alignment_sweep():
    """Per first-item size f = 1 .. 16 bytes (masks; 3 f for frames, 2 f for int16 PCM) one store: a 1 x f item, then items of 16 rows
    and width w = 1 .. 40.  16 rows of w bytes are a multiple of 16, so every later item starts f bytes past a 16-byte boundary and
    its row r at f + r w; the destination rows are 41 (123 for frames) bytes apart, which is odd: over 16 rows every destination
    offset occurs, and over the 16 values of f every source offset with it.  Head, body and tail exact, nothing past a row."""
    from cavp_amd.store import BatchFeeder, FeedResult
    rng = np.random.default_rng(1)
    res = None
    for f in range(1, 17):
        items = [_item(rng, 1, f, [(1, f, 0)], np.int16)] + [_item(rng, 16, w, [(1, w, 0)], np.int16) for w in range(1, 41)]
        st = _make(items, (16, 41), 1, 1, 41, torch.int16)
        fd, ref = BatchFeeder(st, batch=41), R.StoreRef(items, B=41)
        res = FeedResult(41, st, DEV) if res is None else res
        _feed_and_compare(fd, ref, res, index=list(range(41)), what=f"first item of {f} bytes")
        fd.check()


def test_rows_longer_than_one_chunk_and_one_workgroup():
    """Rows of 160 000 bytes (40 chunks of 4 KiB, several workgroups per segment), one of them one sample short and one of odd
    length; a frame that fills its slot (copied as ONE row of 3 * 40 * 64 bytes) beside one that does not."""
    from cavp_amd.store import BatchFeeder, FeedResult
    rng = np.random.default_rng(2)
    items = [_item(rng, 40, 64, [(2, 40000, 0)], np.float32), _item(rng, 40, 63, [(1, 39999, 1)], np.float32),
             _item(rng, 39, 64, [(2, 12345, 0)], np.float32)]
    st = _make(items, (40, 64), 1, 2, 40000, torch.float32)
    fd, ref = BatchFeeder(st, batch=3, seed=1), R.StoreRef(items, B=3, seed=1)
    res = FeedResult(3, st, DEV)
    _feed_and_compare(fd, ref, res, what="draw")
    _feed_and_compare(fd, ref, res, index=[2, 0, 1], what="index")


def test_more_than_one_wave_of_work():
    """N = 300, B = 32, stage 64 x 64: three consecutive steps equal the restatement; index is pi_e at the expected t."""
    from cavp_amd.store import BatchFeeder, FeedResult
    rng = np.random.default_rng(3)
    items = []
    for i in range(300):
        h, w = (64, 64) if i % 10 == 0 else (int(rng.integers(1, 65)), int(rng.integers(1, 65)))
        srcs = [(int(rng.integers(1, 3)), int(rng.integers(1, 3001)), int(rng.integers(0, 4))) for _ in range(int(rng.integers(0, 3)))]
        items.append(_item(rng, h, w, srcs, np.int16))
    st = _make(items, (64, 64), 2, 2, 3000, torch.int16)
    fd, ref = BatchFeeder(st, batch=32, seed=11), R.StoreRef(items, B=32, seed=11)
    assert fd.steps_per_epoch == 9
    fd.set_step(7)                                    # 7, 8 close epoch 0, 9 opens epoch 1
    ref.t = 7
    res = FeedResult(32, st, DEV)
    for t in (7, 8, 9):
        got = _feed_and_compare(fd, ref, res, what=f"step {t}")
        e, s = divmod(t, 9)
        assert got["index"].tolist() == [R.permute(s * 32 + i, 300, 11, e) for i in range(32)]
    assert fd.step() == 10 and fd.state_dict() == {"seed": 11, "t": 10}
    fd.check()


def _tiny_store(N=10):
    rng = np.random.default_rng(4)
    items = [_item(rng, int(rng.integers(1, 5)), int(rng.integers(1, 7)), [(1, int(rng.integers(1, 9)), 0)], np.int16) for _ in range(N)]
    return items, _make(items, (4, 6), 1, 1, 8, torch.int16)


def test_epoch_roll_over_in_a_graph():
    """feed(out=res) captured once with N = 10, B = 4 (spe = 2) and replayed 5 times: index after replay r is step r, t = 0 .. 4
    spans three epochs.  Warm-up behaviour: a capture launches nothing, so it consumes no step; an eager warm-up feed (which loads
    the code object outside the capture) consumes one like any feed, and set_step(0) takes it back."""
    from cavp_amd.store import BatchFeeder, FeedResult
    items, st = _tiny_store()
    fd = BatchFeeder(st, batch=4, seed=2)
    res = FeedResult(4, st, DEV)
    fd.feed(out=res)                                  # warm-up
    assert fd.step() == 1
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fd.feed(out=res)
    torch.cuda.current_stream().wait_stream(side)
    assert fd.step() == 1                             # the capture consumed nothing
    fd.set_step(0)
    ref = R.StoreRef(items, B=4, seed=2)
    for t in range(5):
        _sentinel(res)
        want = ref.feed(_host(res))
        graph.replay()
        torch.cuda.synchronize()
        got = _host(res)
        assert got["index"].tolist() == R.batch_indices(10, 4, 2, t).tolist(), t
        for name in FIELDS:
            assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), (t, name)
    assert fd.step() == 5
    assert [fd.epoch_of(t) for t in range(5)] == [0, 0, 1, 1, 2]


def test_index_override_bad_inputs_and_rollback():
    from cavp_amd._lib import CavpError
    from cavp_amd.rollback import StepRollback
    from cavp_amd.store import BatchFeeder, FeedResult
    items, st = _tiny_store()
    fd, ref = BatchFeeder(st, batch=4, seed=3), R.StoreRef(items, B=4, seed=3)
    res = FeedResult(4, st, DEV)
    got = _feed_and_compare(fd, ref, res, index=[9, 10, -1, 3], what="bad index")
    assert got["index"].tolist() == [9, 0, 0, 3] and ref.bad == 2
    with pytest.raises(CavpError, match="2 input value"):
        fd.check()
    fd.check()                                        # the counter was cleared
    with pytest.raises(CavpError, match="int32"):
        fd.feed(index=torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(CavpError, match="CPU tensor"):
        fd.feed(index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(CavpError, match="other shapes"):
        fd.feed(out=FeedResult(3, st, DEV))
    # a skipped step sees the same batch again
    rb = StepRollback(DEV).add(fd).freeze()
    assert rb.registered_bytes() == {"BatchFeeder.state": 16}
    t0 = fd.step()
    rb.save()
    first = fd.feed().index.clone()
    assert fd.step() == t0 + 1
    rb.restore()
    assert fd.step() == t0
    again = fd.feed(out=res)
    assert torch.equal(first, again.index) and first.tolist() == R.batch_indices(10, 4, 3, t0).tolist()
    # checkpoint round trip
    sd = fd.state_dict()
    nxt = fd.feed().index.clone()
    fd.load_state_dict(sd)
    assert torch.equal(nxt, fd.feed().index)
    fd.manual_seed(8)
    assert fd.state_dict() == {"seed": 8, "t": 0}


def test_two_ranks_in_one_process():
    """world = 2 on one store of N = 11: M = 6 per rank, B = 3, spe = 2.  Per step the two ranks' rows are disjoint, and over an epoch
    they cover all 11 items with exactly one seen twice (the pad)."""
    from cavp_amd.store import BatchFeeder
    items, st = _tiny_store(11)
    fds = [BatchFeeder(st, batch=3, seed=6, rank=r, world=2) for r in (0, 1)]
    for e in range(2):
        seen = []
        for s in range(2):
            rows = [fd.feed().index.cpu().numpy() for fd in fds]
            for r in (0, 1):
                assert rows[r].tolist() == R.batch_indices(11, 3, 6, e * 2 + s, r, 2).tolist()
            both = np.concatenate(rows)
            seen.append(both)
            if len(set(both.tolist())) != 6:          # only the step that holds the pad position may repeat an item
                assert s == 1 and len(set(both.tolist())) == 5
        counts = np.bincount(np.concatenate(seen), minlength=11)
        assert sorted(counts.tolist()) == [1] * 10 + [2]


def test_stages_fed_from_the_store_equal_host_staging():
    """FrameAugment (params= fixed) and WaveStage on a FeedResult equal the same stages on host-staged copies of the same items."""
    from cavp_amd.augment import FrameAugment, make_params
    from cavp_amd.store import BatchFeeder
    from cavp_amd.wave import WaveStage
    rng = np.random.default_rng(5)
    Hs, Ws, S, Cm, Lmax, B = 48, 64, 2, 2, 3000, 4
    items = []
    for i in range(6):
        h, w = int(rng.integers(16, Hs + 1)), int(rng.integers(24, Ws + 1))
        srcs = [(int(rng.integers(1, 3)), int(rng.integers(1500, Lmax + 1)), int(rng.integers(0, 2))) for _ in range(1 + i % 2)]
        items.append(_item(rng, h, w, srcs, np.int16))
    st = _make(items, (Hs, Ws), S, Cm, Lmax, torch.int16)
    fed = BatchFeeder(st, batch=B, seed=1).feed()
    idx = fed.index.cpu().numpy()
    frames, masks = np.zeros((B, Hs, Ws, 3), np.uint8), np.zeros((B, Hs, Ws), np.uint8)
    pcm = np.zeros((B, S, Cm, Lmax), np.int16)
    sizes, length, rate, nch = np.zeros((B, 2), np.int32), np.zeros((B, S), np.int32), np.zeros((B, S), np.int32), np.zeros((B, S), np.int32)
    for b, it in enumerate(idx):
        f, m, srcs = items[int(it)]
        h, w = m.shape
        frames[b, :h, :w], masks[b, :h, :w], sizes[b] = f, m, (h, w)
        for s, (p, r) in enumerate(srcs):
            pcm[b, s, :p.shape[0], :p.shape[1]], length[b, s], rate[b, s], nch[b, s] = p, p.shape[1], r, p.shape[0]
    dev = lambda a: torch.from_numpy(a).to(DEV)
    aug = FrameAugment(crop=(16, 24), jitter=None, seed=0, device=DEV, max_batch=B, stage=(Hs, Ws))
    # scale 1.0 and origin (0, 0): legal for every item size here (each holds the 16 x 24 crop); flip off and on
    params = torch.stack([make_params(b % 2, 2, 0, 0) for b in range(B)]).to(DEV)
    a = aug(fed.frames, fed.masks, fed.sizes, params=params)
    b_ = aug(dev(frames), dev(masks), dev(sizes), params=params)
    aug.check()
    assert torch.equal(a.image, b_.image) and torch.equal(a.label, b_.label)
    ws = WaveStage(audio_len=0.05, rates=(16000, 44100), max_sources=S, max_channels=Cm, max_len=Lmax, device=DEV, max_batch=B)
    x = ws(fed.pcm, fed.length, fed.rate_idx, fed.n_ch)
    y = ws(dev(pcm), dev(length), dev(rate), dev(nch))
    ws.check()
    assert torch.equal(x.waveform, y.waveform) and float(x.waveform.abs().max()) > 0
