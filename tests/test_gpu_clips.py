"""The clip store (cavp_amd/clips.py, csrc/store.hip) against the numpy restatement tests/_clips_ref.py.  Every comparison is
bit-exact.  The restatement writes INTO copies of the buffers as they were before the feed (0xA5 everywhere), so whole-buffer
equality holds the windows to the clips AND everything outside them - empty frame slots, masks of frames without one, absent
channels - to "not written"."""
import numpy as np
import pytest
import torch

from tests import _clips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAIN = ("frames", "masks", "sizes", "pcm", "length", "rate_idx", "n_ch", "index", "select", "tag")
EVAL = ("frames", "masks", "sizes", "pcm", "length", "rate_idx", "n_ch", "index", "count", "n_frames", "tag")
NP = {torch.int16: np.int16, torch.float32: np.float32}


def _clip(rng, sizes, masked, srcs, dtype, avail=None, mask_num=None, tag=0):
    """One clip in the restatement's form.  sizes: [(h, w)] per frame; masked: the frames with a mask; srcs: [(n_ch, len, rate_idx)];
    avail / mask_num default as ClipStore.append's do."""
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    masks = [rng.integers(0, 256, (h, w), dtype=np.uint8) if k in masked else None for k, (h, w) in enumerate(sizes)]
    if dtype is np.int16:
        pcm = [(rng.integers(-32768, 32768, (c, n)).astype(np.int16), r) for c, n, r in srcs]
    else:
        pcm = [(rng.standard_normal((c, n)).astype(np.float32), r) for c, n, r in srcs]
    if avail is None:
        avail = sum(1 << k for k in masked)
    if mask_num is None:
        mask_num = next((k for k in range(len(sizes)) if k not in masked), len(sizes))
    return frames, masks, pcm, avail, mask_num, tag


def _make(clips, stage, T, S, Cm, Lmax, dtype):
    """Even clips go in with explicit available / mask_num, odd ones through append's defaults wherever those give the same values
    (with the masks list cut after its last mask)."""
    from cavp_amd.clips import ClipStore
    st = ClipStore(stage=stage, max_frames=T, max_sources=S, max_channels=Cm, max_len=Lmax, pcm_dtype=dtype, device=DEV)
    for i, (f, m, p, av, mn, tg) in enumerate(clips):
        has = sum(1 << k for k, x in enumerate(m) if x is not None)
        lead = next((k for k, x in enumerate(m) if x is None), len(m))
        if i % 2 and (av, mn) == (has, lead):
            st.append(f, m[:has.bit_length()], p, tag=tg)
        else:
            st.append(f, m, p, available=av, mask_num=mn, tag=tg)
    return st.freeze()


def _sentinel(res, fields):
    """0xA5 into every byte of every output, the tables included."""
    for name in fields:
        getattr(res, name).view(-1).view(torch.uint8).fill_(0xA5)


def _host(res, fields):
    return {name: getattr(res, name).cpu().numpy() for name in fields}


def _same(got, want, fields, what):
    for name in fields:
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), f"{what}: {name}"


def _dev(values):
    return None if values is None else torch.tensor(values, dtype=torch.int32, device=DEV)


def _feed_and_compare(feeder, ref, res, index=None, frame=None, what=""):
    _sentinel(res, TRAIN)
    want = ref.feed(_host(res, TRAIN), index=index, frame=frame)
    feeder.feed(out=res, index=_dev(index), frame=_dev(frame))
    torch.cuda.synchronize()
    got = _host(res, TRAIN)
    _same(got, want, TRAIN, what)
    return got


def _eval_and_compare(feeder, ref, res, what=""):
    _sentinel(res, EVAL)
    want = ref.feed_clips(_host(res, EVAL))
    feeder.feed_clips(out=res)
    torch.cuda.synchronize()
    got = _host(res, EVAL)
    _same(got, want, EVAL, what)
    return got


STAGE, TMAX, S, CM, LMAX = (40, 56), 10, 2, 2, 4097
_SIZES = [(7, 17), (40, 5), (1, 56), (7, 56), (40, 1), (1, 1), (7, 5), (40, 56), (1, 17), (40, 17)]


def _shared_clips(dtype):
    """N = 7 on a 40 x 56 stage, Tmax = 10: n_frames in {1, 3, 5, 10}; widths 1, 5, 17, 56 (rows shorter than 16 bytes, rows that
    straddle one boundary, whole staging rows: the w == Ws path) and heights 1, 7, 40; frames without masks in the middle and at the
    end of a clip; 0, 1 or 2 sources of 1 or 2 channels, 1 / 15 / 16 / 17 / 4097 samples."""
    rng = np.random.default_rng(0)
    c = lambda *a, **k: _clip(rng, *a, dtype=dtype, **k)
    return [c([(1, 1)], {0}, [(1, 1, 0)], tag=-5),
            c([(7, 5), (40, 56), (1, 17)], {0, 1, 2}, [(2, 15, 1), (1, 16, 0)], tag=2),
            c(_SIZES[:5], {0, 2, 3}, [(2, 17, 2)], tag=1),
            c(_SIZES, {0, 1, 2, 3, 4, 7}, [(1, 4097, 0), (2, 4097, 1)], avail=0b10010101, mask_num=5, tag=4),
            c([(40, 56)] * 10, set(range(10)), [], tag=7),
            c([(7, 5)] * 3, {2}, [(1, 16, 3)], tag=10),
            c([(40, 56)], {0}, [(2, 1, 0)], tag=13)]


@pytest.fixture(scope="module", params=[torch.int16, torch.float32], ids=["int16", "float32"])
def shared(request):
    dtype = request.param
    clips = _shared_clips(NP[dtype])
    return clips, _make(clips, STAGE, TMAX, S, CM, LMAX, dtype)


def test_train_feed_equals_the_restatement(shared):
    """B = 4 over 3 epochs of N = 7 (spe = 1), then every clip and every drawable frame once more through index= / frame=, so that
    each special size is gathered whatever the draws were; clip(i) reads back what was appended."""
    from cavp_amd.clips import ClipFeeder, ClipFeedResult
    clips, st = shared
    for i, (f, m, p, av, mn, tg) in enumerate(clips):
        gf, gm, gp, ga, gn, gt = st.clip(i)
        assert all(np.array_equal(a, b) for a, b in zip(gf, f)) and len(gf) == len(f) and (ga, gn, gt) == (av, mn, tg)
        assert all((a is None) == (b is None) and (b is None or np.array_equal(a, b)) for a, b in zip(gm, m))
        assert all(np.array_equal(a, b) and ra == rb for (a, ra), (b, rb) in zip(gp, p)) and len(gp) == len(p)
    fd, ref = ClipFeeder(st, batch=4, seed=5), R.ClipsRef(clips, B=4, Tmax=TMAX, seed=5)
    assert fd.steps_per_epoch == 1
    res = ClipFeedResult(4, st, DEV)
    for t in range(3):
        got = _feed_and_compare(fd, ref, res, what=f"step {t}")
        assert got["index"].tolist() == R.batch_indices(7, 4, 5, t).tolist()
        assert got["select"].tolist() == [R.draw_frame(clips[c][3], 5, t, i) for i, c in enumerate(got["index"])]
    assert fd.step() == 3 and fd.eval_step() == 0
    for idx, frm in (([0, 1, 2, 3], [0, 1, 2, 7]), ([4, 5, 6, 1], [9, 2, 0, 2]), ([3, 3, 3, 2], [0, 2, 4, 3]), ([1, 2, 4, 4], [0, 0, 5, 0])):
        _feed_and_compare(fd, ref, res, index=idx, frame=frm, what=f"index {idx} frame {frm}")
    _feed_and_compare(fd, ref, res, index=[3, 3, 2, 2], what="index alone: the frames are drawn")
    fd.check()


@pytest.mark.parametrize("world", [1, 2])
def test_eval_feed_equals_the_restatement(shared, world):
    """Two passes over N = 7 at B = 4: world = 1 has P = 2 steps per pass (the second with a padding row), world = 2 has P = 1 and one
    padding row on rank 1; both ranks are two feeders in one process.  Across the ranks every clip is scored once per pass."""
    from cavp_amd.clips import ClipEvalResult, ClipFeeder
    clips, st = shared
    fds = [ClipFeeder(st, batch=4, seed=1, rank=r, world=world) for r in range(world)]
    refs = [R.ClipsRef(clips, B=4, Tmax=TMAX, seed=1, rank=r, world=world) for r in range(world)]
    P = fds[0].steps_per_pass
    assert P == 3 - world
    res = ClipEvalResult(4, st, DEV)
    for p in range(2):
        seen = []
        for s in range(P):
            for r in range(world):
                got = _eval_and_compare(fds[r], refs[r], res, what=f"pass {p} step {s} rank {r}")
                pad = got["index"] < 0
                assert (got["count"][pad] == 0).all() and got["count"][~pad].tolist() == [clips[c][4] for c in got["index"][~pad]]
                seen += got["index"][~pad].tolist()
        assert sorted(seen) == list(range(7))
    assert fds[0].eval_step() == 2 * P and fds[0].step() == 0
    fds[0].check()


def test_alignment_sweep():
    """The same clip behind a filler clip of f = 0 .. 15 mask bytes (3 f frame bytes: every residue mod 16, 3 being odd; 2 f PCM
    bytes: every even residue, and int16 rows are never odd): every source misalignment of frame, mask and PCM rows, against
    destination rows 56 * 3 = 168 and 56 bytes apart (8 mod 16: two destination phases per window) and the whole-window path."""
    from cavp_amd.clips import ClipEvalResult, ClipFeeder, ClipFeedResult
    rng = np.random.default_rng(1)
    clip = _clip(rng, [(7, 17), (40, 5), (3, 56), (5, 1)], {0, 1, 2, 3}, [(2, 33, 0), (1, 4097, 1)], np.int16, tag=3)
    res = ev = None
    for f in range(16):
        clips = ([_clip(rng, [(1, f)], {0}, [(1, f, 0)], np.int16)] if f else []) + [clip]
        st = _make(clips, STAGE, 4, S, CM, LMAX, torch.int16)
        assert st.arena_bytes()["masks"] == f + clip[1][0].size + clip[1][1].size + clip[1][2].size + clip[1][3].size
        fd, ref = ClipFeeder(st, batch=1), R.ClipsRef(clips, B=1, Tmax=4)
        res = ClipFeedResult(1, st, DEV) if res is None else res
        ev = ClipEvalResult(1, st, DEV) if ev is None else ev
        for k in range(4):
            _feed_and_compare(fd, ref, res, index=[len(clips) - 1], frame=[k], what=f"filler {f} frame {k}")
        for s in range(len(clips)):
            _eval_and_compare(fd, ref, ev, what=f"filler {f} eval step {s}")
        fd.check()


def test_rows_longer_than_one_chunk_and_one_workgroup():
    """One clip whose frame fills the 40 x 56 slot (ONE row of 6720 bytes: two 4 KiB chunks) and whose PCM rows are 70 000 float32
    samples (280 000 bytes: 69 chunks over 9 workgroups), behind an odd number of bytes."""
    from cavp_amd.clips import ClipEvalResult, ClipFeeder, ClipFeedResult
    rng = np.random.default_rng(2)
    clips = [_clip(rng, [(1, 3)], {0}, [(1, 5, 0)], np.float32), _clip(rng, [(40, 56), (40, 55)], {0, 1}, [(2, 70000, 0)], np.float32)]
    st = _make(clips, STAGE, 2, 1, 2, 70000, torch.float32)
    fd, ref = ClipFeeder(st, batch=2, seed=1), R.ClipsRef(clips, B=2, Tmax=2, seed=1)
    res, ev = ClipFeedResult(2, st, DEV), ClipEvalResult(2, st, DEV)
    _feed_and_compare(fd, ref, res, what="draw")
    _feed_and_compare(fd, ref, res, index=[1, 1], frame=[0, 1], what="override")
    _eval_and_compare(fd, ref, ev, what="eval")


def test_overrides_bad_inputs_and_rollback(shared):
    from cavp_amd._lib import CavpError
    from cavp_amd.clips import ClipEvalResult, ClipFeeder, ClipFeedResult
    from cavp_amd.rollback import StepRollback
    clips, st = shared
    fd, ref = ClipFeeder(st, batch=4, seed=3), R.ClipsRef(clips, B=4, Tmax=TMAX, seed=3)
    res = ClipFeedResult(4, st, DEV)
    # index 7 and -1 become clip 0 (whose only frame is 0: frame 3 there is bad too); clip 3 has avail 0b10010101: frame 1 is not
    # in it (-> 0), frame 7 is; frame 32 and -1 are outside any mask
    got = _feed_and_compare(fd, ref, res, index=[3, 7, -1, 3], frame=[1, 3, 0, 7], what="bad index / frame")
    assert got["index"].tolist() == [3, 0, 0, 3] and got["select"].tolist() == [0, 0, 0, 7] and ref.bad == 4
    got = _feed_and_compare(fd, ref, res, index=[5, 5, 2, 2], frame=[32, -1, 1, 2], what="bad frame")
    assert got["select"].tolist() == [2, 2, 0, 2] and ref.bad == 7
    with pytest.raises(CavpError, match="7 input value"):
        fd.check()
    fd.check()                                        # the counter was cleared
    with pytest.raises(CavpError, match="int32"):
        fd.feed(frame=torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(CavpError, match="CPU tensor"):
        fd.feed(index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(CavpError, match="other shapes"):
        fd.feed(out=ClipFeedResult(3, st, DEV))
    with pytest.raises(CavpError, match="other shapes"):
        fd.feed_clips(out=res)
    with pytest.raises(CavpError, match="no full batch"):
        ClipFeeder(st, batch=8).feed()
    with pytest.raises(CavpError, match="batch \\* max_frames"):
        ClipFeeder(st, batch=128).feed_clips()
    # a skipped step sees the same clips and the same frames again; an eval step in between moves neither
    rb = StepRollback(DEV).add(fd).freeze()
    assert list(rb.registered_bytes().values()) == [16]
    t0 = fd.step()
    rb.save()
    first = fd.feed()
    first = (first.index.clone(), first.select.clone())
    fd.feed_clips()
    assert fd.step() == t0 + 1 and fd.eval_step() == 1
    rb.restore()
    assert fd.step() == t0 and fd.eval_step() == 1
    again = fd.feed(out=res)
    assert torch.equal(first[0], again.index) and torch.equal(first[1], again.select)
    assert first[0].tolist() == R.batch_indices(7, 4, 3, t0).tolist()
    assert first[1].tolist() == [R.draw_frame(clips[c][3], 3, t0, i) for i, c in enumerate(first[0].tolist())]
    # checkpoint round trip
    sd = fd.state_dict()
    assert sd == {"seed": 3, "t": t0 + 1, "t_eval": 1}
    nxt, nxt_ev = fd.feed().select.clone(), fd.feed_clips().index.clone()
    fd.load_state_dict(sd)
    assert torch.equal(nxt, fd.feed().select) and torch.equal(nxt_ev, fd.feed_clips().index)
    fd.manual_seed(8)
    assert fd.state_dict() == {"seed": 8, "t": 0, "t_eval": 2}       # manual_seed leaves the eval counter where it is
    assert isinstance(fd.feed_clips(), ClipEvalResult)


def _capture(fn):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def test_both_feeds_in_a_graph(shared):
    """feed(out=) and feed_clips(out=) each captured once and replayed across an epoch / a pass boundary (N = 7, B = 3: spe = 2, P =
    3); after every replay the buffers equal those of an eager feed from a second feeder with the same seed, and the restatement's
    indices.  A capture launches nothing, so it consumes no step; the eager warm-up feeds do, and set_step takes them back."""
    from cavp_amd.clips import ClipEvalResult, ClipFeeder, ClipFeedResult
    clips, st = shared
    fd, eager = ClipFeeder(st, batch=3, seed=2), ClipFeeder(st, batch=3, seed=2)
    res, res2 = ClipFeedResult(3, st, DEV), ClipFeedResult(3, st, DEV)
    ev, ev2 = ClipEvalResult(3, st, DEV), ClipEvalResult(3, st, DEV)
    fd.feed(out=res)                                  # warm-up: the code objects are loaded outside the captures
    fd.feed_clips(out=ev)
    g_train = _capture(lambda: fd.feed(out=res))
    g_eval = _capture(lambda: fd.feed_clips(out=ev))
    assert (fd.step(), fd.eval_step()) == (1, 1)
    fd.set_step(0, 0)
    for t in range(5):                                # epochs 0, 0, 1, 1, 2
        _sentinel(res, TRAIN)
        _sentinel(res2, TRAIN)
        g_train.replay()
        eager.feed(out=res2)
        torch.cuda.synchronize()
        _same(_host(res, TRAIN), _host(res2, TRAIN), TRAIN, f"train replay {t}")
        assert res.index.tolist() == R.batch_indices(7, 3, 2, t).tolist()
        assert res.select.tolist() == [R.draw_frame(clips[c][3], 2, t, i) for i, c in enumerate(res.index.tolist())]
    for t in range(4):                                # pass 0: steps 0, 1, 2; step 3 opens pass 1
        _sentinel(ev, EVAL)
        _sentinel(ev2, EVAL)
        g_eval.replay()
        eager.feed_clips(out=ev2)
        torch.cuda.synchronize()
        _same(_host(ev, EVAL), _host(ev2, EVAL), EVAL, f"eval replay {t}")
        assert ev.index.tolist() == [c if not pad else -1 for c, pad in R.eval_rows(7, 3, t)]
    assert (fd.step(), fd.eval_step()) == (5, 4)


def test_stages_fed_from_the_clip_store_equal_host_staging():
    """FrameAugment (params= fixed) + WaveStage(segments=T, select=fed.select) on a fed batch equal the same stages on buffers staged
    by hand from the selected frames; FrameAugment.eval_ + ClipValidation.update(mask, labels, ev.count) on a fed pass equal the same
    calls on hand-staged clips (a random uint8 "prediction" mask): exactly equal outputs, equal integer counts."""
    from cavp_amd.augment import FrameAugment, make_params
    from cavp_amd.clips import ClipFeeder
    from cavp_amd.metrics import ClipValidation
    from cavp_amd.wave import WaveStage
    rng = np.random.default_rng(5)
    Hs, Ws, T, Lmax, B, K = 48, 64, 5, 3200, 4, 3
    clips = []
    for i in range(6):
        n = (5, 3, 1, 5, 2, 4)[i]
        sizes = [(int(rng.integers(16, Hs + 1)), int(rng.integers(24, Ws + 1))) for _ in range(n)]
        masked = set(range(n)) - ({1} if n > 2 else set())
        clip = _clip(rng, sizes, masked, [(1 + i % 2, int(rng.integers(1600, Lmax + 1)), i % 2)], np.int16, tag=i)
        for m in clip[1]:
            if m is not None:
                m[...] = rng.choice(np.array([0, 1, 2, 255], np.uint8), m.shape)        # class indices and the ignore value
        clips.append(clip)
    st = _make(clips, (Hs, Ws), T, 1, 2, Lmax, torch.int16)
    fd = ClipFeeder(st, batch=B, seed=1)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    zeros = lambda res, fields: {k: np.zeros_like(v) for k, v in _host(res, fields).items()}
    aug = FrameAugment(crop=(16, 24), jitter=None, seed=0, device=DEV, max_batch=B * T, stage=(Hs, Ws))
    ws = WaveStage(audio_len=0.1, rates=(16000, 44100), max_sources=1, max_channels=2, max_len=Lmax, segments=T, device=DEV, max_batch=B)
    # ---- training: one frame per row
    fed = fd.feed()
    hand = R.ClipsRef(clips, B=B, Tmax=T).feed(zeros(fed, TRAIN), index=fed.index.cpu().numpy(), frame=fed.select.cpu().numpy())
    assert np.array_equal(hand["frames"], fed.frames.cpu().numpy()) and len(set(fed.select.tolist())) > 1
    params = torch.stack([make_params(b % 2, 2, 0, 0) for b in range(B)]).to(DEV)      # scale 1.0, origin (0, 0), flip off / on
    a = aug(fed.frames, fed.masks, fed.sizes, params=params)
    a = (a.image.clone(), a.label.clone())
    b_ = aug(dev(hand["frames"]), dev(hand["masks"]), dev(hand["sizes"]), params=params)
    assert torch.equal(a[0], b_.image) and torch.equal(a[1], b_.label)
    x = ws(fed.pcm, fed.length, fed.rate_idx, fed.n_ch, select=fed.select).waveform.clone()
    y = ws(dev(hand["pcm"]), dev(hand["length"]), dev(hand["rate_idx"]), dev(hand["n_ch"]), select=dev(hand["select"])).waveform
    ws.check()
    assert torch.equal(x, y) and float(x.abs().max()) > 0 and tuple(x.shape) == (B, 1, 1600 // T)
    # ---- validation: whole clips in order, two steps = one pass
    cv, cv_hand = (ClipValidation(num_classes=K, ignore_index=255, min_count=10, min_values=2, max_frames=B * T, device=DEV) for _ in range(2))
    ref = R.ClipsRef(clips, B=B, Tmax=T)
    assert fd.steps_per_pass == 2
    for s in range(2):
        ev = fd.feed_clips()
        hand = ref.feed_clips(zeros(ev, EVAL))
        pred = torch.from_numpy(rng.integers(0, K, (B * T, 16, 24), dtype=np.uint8)).to(DEV)
        e = aug.eval_(ev.frames.view(B * T, Hs, Ws, 3), ev.masks.view(B * T, Hs, Ws), ev.sizes)
        image, labels = e.image.clone(), e.label.clone().view(B, T, 16, 24)
        cv.update(pred, labels, ev.count)
        h = aug.eval_(dev(hand["frames"]).view(B * T, Hs, Ws, 3), dev(hand["masks"]).view(B * T, Hs, Ws), dev(hand["sizes"]))
        assert torch.equal(image, h.image) and torch.equal(labels.view(B * T, 16, 24), h.label)
        cv_hand.update(pred, h.label.view(B, T, 16, 24), dev(hand["count"]))
    aug.check()
    cv.check()
    got, want = cv.counts().cpu(), cv_hand.counts().cpu()
    assert torch.equal(got, want) and int(got.sum()) > 0
