"""CPU-side checks of the clip store (cavp_amd/clips.py, csrc/store.hip) on the numpy restatement tests/_clips_ref.py alone: the
packed tables read back what was appended, append() fails loudly, the frame draw is uniform over the set bits of `avail`, the eval
walk visits every clip once per pass across ranks, the two counters are independent, and the library, the header and the ctypes
table agree."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _clips_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_clips_plan_words", "cavp_clips_plan_train", "cavp_clips_plan_eval", "cavp_clips_gather")


def test_library_exports_the_clip_entry_points():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    bound = _lib.load()
    assert _lib.ABI_VERSION == bound.cavp_abi_version()
    assert bound.cavp_clips_plan_words(1, 3) == 4 + 3 * 3 == bound.cavp_store_plan_words(3)
    assert bound.cavp_clips_plan_words(10, 2) == 40 + 6


def test_header_and_ctypes_table_agree():
    from cavp_amd import _lib, clips
    text = open(os.path.join(REPO, "include", "cavp_hip.h")).read()
    as_ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/cavp_hip.h"
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if "*" in arg else as_ctype[arg.replace("const ", "").split(" ")[0]])
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == want, name
    assert int(re.search(r"#define CAVP_CLIPS_MAX_FRAMES (\d+)", text).group(1)) == clips.MAX_FRAMES


def test_store_module_re_exports_the_clip_classes():
    from cavp_amd import clips, store
    for name in ("ClipStore", "ClipFeeder", "ClipFeedResult", "ClipEvalResult"):
        assert getattr(store, name) is getattr(clips, name)
    with pytest.raises(AttributeError):
        store.NoSuchClass


# ---- the host API ------------------------------------------------------------------------------------------------------------------
def _clip(rng, sizes, masked, srcs, dtype=np.int16):
    """sizes: [(h, w)] per frame; masked: the frames that get a mask; srcs: [(n_ch, len, rate_idx)]"""
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    masks = [rng.integers(0, 256, (h, w), dtype=np.uint8) if k in masked else None for k, (h, w) in enumerate(sizes)]
    pcm = [(rng.integers(-32768, 32768, (c, n)).astype(dtype), r) for c, n, r in srcs]
    return frames, masks, pcm


def _store(**kw):
    from cavp_amd.clips import ClipStore
    args = dict(stage=(8, 12), max_frames=5, max_sources=2, max_channels=2, max_len=40, pcm_dtype=torch.int16)
    args.update(kw)
    return ClipStore(**args)


def _same_clip(got, frames, masks, pcm, avail, mask_num, tag):
    gf, gm, gp, ga, gn, gt = got
    assert len(gf) == len(frames) and len(gm) == len(frames) and len(gp) == len(pcm)
    for k, f in enumerate(frames):
        assert np.array_equal(gf[k], f), k
        m = masks[k] if k < len(masks) else None
        assert (gm[k] is None) == (m is None) and (m is None or np.array_equal(gm[k], m)), k
    assert all(np.array_equal(a, b) and ra == rb for (a, ra), (b, rb) in zip(gp, pcm))
    assert (ga, gn, gt) == (avail, mask_num, tag)


def test_pack_round_trips_through_clip_before_the_upload():
    """Defaults: available = the frames with a mask, mask_num = the leading frames with one; a shorter masks list; explicit values;
    a frame without a mask takes no byte of the mask arena and has mask_off = -1.  Before and after freeze(upload=False)."""
    rng = np.random.default_rng(0)
    st = _store()
    a = _clip(rng, [(8, 12), (3, 5), (1, 1)], {0, 1, 2}, [(2, 40, 1)])
    b = _clip(rng, [(2, 7)] * 5, {0, 1, 3}, [])
    c = _clip(rng, [(4, 4), (5, 6)], {0}, [(1, 3, 0), (2, 9, 2)])
    assert st.append(*a) == 0
    assert st.append(*b, tag=7) == 1
    assert st.append(c[0], c[1][:1], c[2], available=[1], mask_num=0, tag=-3) == 2       # masks shorter than frames
    assert st.append(*a, available=0b101, mask_num=2) == 3
    want = [(a, 0b111, 3, 0), (b, 0b1011, 2, 7), (c, 0b1, 0, -3), (a, 0b101, 2, 0)]
    for when in ("appended", "frozen"):
        for i, ((f, m, p), av, mn, tg) in enumerate(want):
            _same_clip(st.clip(i), f, m, p, av, mn, tg)
        if when == "appended":
            t = st.pack()
            st.freeze(upload=False)
    assert len(st) == 4 and st.total_frames == 13
    assert t["first"].tolist() == [0, 3, 8, 10] and t["n_frames"].tolist() == [3, 5, 2, 3] and t["avail"].dtype == np.uint32
    assert t["mask_off"][3 + 2] == -1 and t["mask_off"][3 + 4] == -1 and t["mask_off"][8 + 1] == -1 and (t["mask_off"] == -1).sum() == 3
    assert t["mask_off"][3 + 3] == t["mask_off"][3 + 1] + 14                               # packed back to back across the gap
    assert st.arena_bytes() == {"frames": 3 * sum(f.shape[0] * f.shape[1] for x in (a, b, c, a) for f in x[0]),
                                "masks": sum(m.size for x in (a, b, c, a) for m in x[1] if m is not None),
                                "pcm": 2 * sum(p.size for x in (a, b, c, a) for p, _ in x[2])}
    assert st.nbytes == sum(st.arena_bytes().values()) + 13 * (8 + 8 + 8) + 4 * 6 * 4 + 4 * 2 * (8 + 4 + 4 + 4)
    with pytest.raises(Exception, match="frozen"):
        st.append(*a)


def test_append_fails_loudly():
    from cavp_amd._lib import CavpError
    rng = np.random.default_rng(1)
    f, m, p = _clip(rng, [(4, 4), (4, 4), (4, 4)], {0, 2}, [(1, 8, 0)])
    st = _store()
    with pytest.raises(CavpError, match="without a mask"):
        st.append(f, m, p, available=[1, 1, 0])
    with pytest.raises(CavpError, match="without a mask"):
        st.append(f, m, p, available=0b010)
    with pytest.raises(CavpError, match="available is empty"):
        st.append(f, m, p, available=[0, 0, 0])
    with pytest.raises(CavpError, match="available is empty"):
        st.append(f, [None] * 3, p)
    with pytest.raises(CavpError, match="outside the clip"):
        st.append(f, m, p, available=0b1000)
    with pytest.raises(CavpError, match="mask_num = 2 exceeds the 1 leading"):
        st.append(f, m, p, mask_num=2)
    with pytest.raises(CavpError, match="mask_num"):
        st.append(f, m, p, mask_num=-1)
    with pytest.raises(CavpError, match="frames"):
        st.append([], [], p)
    with pytest.raises(CavpError, match="max_frames"):
        st.append(f * 2, m * 2, p)
    with pytest.raises(CavpError, match="masks for"):
        st.append(f[:1], m[:1] + m[:1], p)
    with pytest.raises(CavpError, match=r"uint8 \[h, w, 3\]"):
        st.append([f[0].astype(np.float32)], m[:1], p)
    with pytest.raises(CavpError, match=r"uint8 \[h, w, 3\]"):
        st.append([f[0][:, :, 0]], m[:1], p)
    with pytest.raises(CavpError, match="does not fit the stage"):
        st.append([np.zeros((9, 4, 3), np.uint8)], [np.zeros((9, 4), np.uint8)], p)
    with pytest.raises(CavpError, match=r"mask 0 must be uint8 \[4, 4\]"):
        st.append(f[:1], [np.zeros((4, 5), np.uint8)], p)
    with pytest.raises(CavpError, match="mask 0 must be uint8"):
        st.append(f[:1], [np.zeros((4, 4), np.int32)], p)
    with pytest.raises(CavpError, match="pcm must be int16"):
        st.append(f, m, [(np.zeros((1, 8), np.float32), 0)])
    with pytest.raises(CavpError, match="max_sources"):
        st.append(f, m, p * 3)
    with pytest.raises(CavpError, match="outside"):
        st.append(f, m, [(np.zeros((1, 41), np.int16), 0)])
    with pytest.raises(CavpError, match="device tensor|numpy array"):
        st.append(["frame"], m[:1], p)
    assert len(st) == 0
    with pytest.raises(CavpError, match="empty"):
        st.freeze(upload=False)
    for kw in (dict(max_frames=0), dict(max_frames=33), dict(stage=(0, 4)), dict(max_sources=0), dict(pcm_dtype=torch.float64)):
        with pytest.raises(CavpError):
            _store(**kw)


def test_feeder_limits_touch_no_device():
    from cavp_amd._lib import CavpError
    from cavp_amd.clips import ClipFeeder
    rng = np.random.default_rng(2)
    st = _store()
    for _ in range(7):
        st.append(*_clip(rng, [(2, 2)], {0}, []))
    fd = ClipFeeder(st, batch=4, rank=1, world=2)
    assert (fd.steps_per_epoch, fd.steps_per_pass) == (1, 1)
    fd = ClipFeeder(st, batch=4)
    assert (fd.steps_per_epoch, fd.steps_per_pass) == (1, 2) == (fd.steps_per_epoch, R.steps_per_pass(7, 4))
    assert ClipFeeder(st, batch=8).steps_per_epoch == 0          # eval only: feed() would raise, feed_clips() walks one step
    for kw in (dict(batch=0), dict(batch=1025), dict(batch=2, rank=2, world=2), dict(batch=1, world=8)):
        with pytest.raises(CavpError):
            ClipFeeder(st, **kw)
    with pytest.raises(CavpError, match="ClipStore"):
        ClipFeeder(object(), batch=1)


# ---- the frame draw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1234])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 10])
def test_frame_draw_is_uniform_over_the_set_bits(n, seed):
    """1024 steps x 4 rows per (n, seed): with n = 1 always the one set bit; otherwise every frame's count within 4 standard
    deviations of the binomial mean (4096 / n, sigma = sqrt(4096 * (1/n) * (1 - 1/n)))."""
    avail = (1 << n) - 1
    draws = np.array([R.draw_frame(avail, seed, t, i) for t in range(1024) for i in range(4)])
    counts = np.bincount(draws, minlength=n)
    assert counts.sum() == 4096 and len(counts) == n
    if n == 1:
        assert counts[0] == 4096
        return
    mean, sigma = 4096 / n, (4096 * (1 / n) * (1 - 1 / n)) ** 0.5
    worst = np.abs(counts - mean).max() / sigma
    print(f"n = {n}, seed = {seed}: worst deviation {worst:.2f} sigma")
    assert worst <= 4.0, (counts.tolist(), worst)


def test_sparse_avail_only_yields_set_bits():
    for avail in (0b1000100001, 1 << 31, 0b110, (1 << 31) | 1):
        bits = R.set_bits(avail)
        seen = {R.draw_frame(avail, 5, t, i) for t in range(256) for i in range(4)}
        assert seen == set(bits), (avail, seen)
    # rows and steps draw independently of each other: not one value per step, not one value per row
    d = np.array([[R.draw_frame(0b11111, 0, t, i) for i in range(4)] for t in range(64)])
    assert (d[:, 0] != d[:, 1]).any() and (d[0] != d[1]).any()
    # the counter's high word takes part
    assert [R.draw_frame(0x3FF, 0, t, 0) for t in range(32)] != [R.draw_frame(0x3FF, 0, t + (1 << 32), 0) for t in range(32)]


# ---- the eval walk and the counters ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_eval_walk_visits_every_clip_once_per_pass(world):
    N, B = 7, 4
    P = R.steps_per_pass(N, B, world)
    assert P == (2 if world == 1 else 1)
    seen, pads = [], 0
    for s in range(P):
        for rank in range(world):
            for clip, pad in R.eval_rows(N, B, s, rank, world):
                if pad:
                    assert clip == 0
                    pads += 1
                else:
                    seen.append(clip)
    assert sorted(seen) == list(range(N)) and pads == P * B * world - N
    for rank in range(world):
        assert R.eval_rows(N, B, P, rank, world) == R.eval_rows(N, B, 0, rank, world)       # step P wraps to step 0
    if world == 1:
        assert R.eval_rows(N, B, 0) == [(0, False), (1, False), (2, False), (3, False)]    # in order
        assert R.eval_rows(N, B, 1) == [(4, False), (5, False), (6, False), (0, True)]


def _buffers(B, T, Hs=8, Ws=12, S=2, Cm=2, Lmax=40, train=True):
    z = lambda shape, dt: np.full(shape, 0x5A, dt)
    buf = {"pcm": z((B, S, Cm, Lmax), np.int16), "length": z((B, S), np.int32), "rate_idx": z((B, S), np.int32), "n_ch": z((B, S), np.int32),
           "index": z(B, np.int32), "tag": z(B, np.int32)}
    if train:
        buf.update(frames=z((B, Hs, Ws, 3), np.uint8), masks=z((B, Hs, Ws), np.uint8), sizes=z((B, 2), np.int32), select=z(B, np.int32))
    else:
        buf.update(frames=z((B, T, Hs, Ws, 3), np.uint8), masks=z((B, T, Hs, Ws), np.uint8), sizes=z((B * T, 2), np.int32),
                   count=z(B, np.int32), n_frames=z(B, np.int32))
    return buf


def test_padding_rows_and_independent_counters():
    rng = np.random.default_rng(3)
    clips = []
    for i in range(7):
        n = (1, 3, 5, 2, 4, 5, 1)[i]
        f, m, p = _clip(rng, [(2 + i % 3, 3 + i)] * n, set(range(n)) - ({1} if n > 2 else set()), [(1, 5 + i, 0)])
        clips.append((f, m, p, sum(1 << k for k in range(n) if m[k] is not None), 1 if n > 2 else n, 10 + i))
    ref = R.ClipsRef(clips, B=4, Tmax=5, seed=9)
    ev = ref.feed_clips(_buffers(4, 5, train=False))
    assert ev["index"].tolist() == [0, 1, 2, 3] and ev["count"].tolist() == [1, 1, 1, 2] and ev["n_frames"].tolist() == [1, 3, 5, 2]
    assert (ref.t, ref.t_eval) == (0, 1)                                  # the train counter is untouched by an eval step
    first = ref.feed(_buffers(4, 5))["index"].copy()
    assert (ref.t, ref.t_eval) == (1, 1)                                  # and the reverse
    ev = ref.feed_clips(_buffers(4, 5, train=False))
    assert ev["index"].tolist() == [4, 5, 6, -1] and ev["count"].tolist() == [1, 1, 1, 0]
    assert ev["n_frames"][3] == 1 and ev["tag"].tolist() == [14, 15, 16, 10]      # the padding row is fed clip 0
    assert np.array_equal(ev["frames"][3, 0, :2, :3], clips[0][0][0]) and (ev["frames"][3, 1:] == 0x5A).all()
    assert ev["sizes"].reshape(4, 5, 2)[3].tolist() == [[2, 3]] * 5
    assert (ev["masks"][1, 1] == 0x5A).all() and not (ev["frames"][1, 1, :4, :8] == 0x5A).all()   # clip 5, frame 1: no mask
    # two eval steps in between did not move the training stream
    again = R.ClipsRef(clips, B=4, Tmax=5, seed=9)
    assert again.feed(_buffers(4, 5))["index"].tolist() == first.tolist() == R.batch_indices(7, 4, 9, 0).tolist()
    assert ref.feed_clips(_buffers(4, 5, train=False))["index"].tolist() == [0, 1, 2, 3]  # the third eval step opens the next pass
