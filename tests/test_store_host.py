"""CPU-side checks of the device store (cavp_amd/store.py, csrc/store.hip) on the numpy restatement tests/_store_ref.py alone: the
keyed permutation is a bijection, an epoch visits what RandomSampler / DistributedSampler with drop_last visit, the permutation is
uniform by the statistic of the pair builder's test, the library, the header and the ctypes table agree, and the host API fails
loudly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _store_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_store_plan_words", "cavp_store_plan", "cavp_store_gather")


def test_library_exports_the_store_entry_points():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    bound = _lib.load()
    assert _lib.ABI_VERSION == bound.cavp_abi_version()
    assert bound.cavp_store_plan_words(3) == 4 + 3 * 3
    assert "store.hip" in build.SOURCES


def test_header_and_ctypes_table_agree():
    from cavp_amd import _lib, store
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
    assert int(re.search(r"#define CAVP_STORE_MAX_STAGE (\d+)", text).group(1)) == store.MAX_STAGE


def test_a_library_without_the_symbols_fails_with_the_name(monkeypatch):
    """load() binds every prototype: a symbol the library does not export is named in the error."""
    from cavp_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.PROTOTYPES, "cavp_store_no_such_entry", (ctypes.c_int32, []))
    with pytest.raises(_lib.CavpError, match="cavp_store_no_such_entry"):
        _lib.load()


# ---- the permutation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", [0, 1, (1 << 32) + 5])
def test_permutation_is_a_bijection(epoch):
    for N in list(range(1, 71)) + [1000]:
        got = R.permute_many(np.arange(N), N, seed=7, epoch=epoch)
        assert sorted(got.tolist()) == list(range(N)), N


def test_vector_and_scalar_restatement_agree():
    for N, seed, epoch in ((1, 0, 0), (5, 1, 3), (13, -2, 1 << 33), (64, 1 << 40, 9), (65, 3, 2), (1000, 11, 4)):
        xs = np.arange(N)[:: max(1, N // 16)]
        assert R.permute_many(xs, N, seed, epoch).tolist() == [R.permute(int(x), N, seed, epoch) for x in xs]


def test_epochs_differ_and_seeds_differ():
    a = R.permute_many(np.arange(1000), 1000, 1, 0)
    assert (a != R.permute_many(np.arange(1000), 1000, 1, 1)).mean() > 0.9
    assert (a != R.permute_many(np.arange(1000), 1000, 2, 0)).mean() > 0.9


def test_one_epoch_visits_every_item_once():
    seen = R.epoch_indices(10, 2, seed=3, epoch=4)
    assert sorted(seen.tolist()) == list(range(10))


def test_drop_last_leaves_out_exactly_one_item():
    assert R.steps_per_epoch(11, 2) == 5
    seen = R.epoch_indices(11, 2, seed=3, epoch=0)
    assert len(seen) == 10 and len(set(seen.tolist())) == 10 and set(seen.tolist()) < set(range(11))


def test_two_ranks_cover_everything_with_one_pad():
    """world = 2, N = 5: M = 3 per rank, B = 3: the six draws are the five items and one of them a second time."""
    both = np.concatenate([R.epoch_indices(5, 3, seed=9, epoch=2, rank=r, world=2) for r in (0, 1)])
    counts = np.bincount(both, minlength=5)
    assert len(both) == 6 and sorted(counts.tolist()) == [1, 1, 1, 1, 2]


def test_steps_run_through_the_epochs():
    N, B = 10, 4                                  # spe = 2: t = 0, 1 epoch 0; t = 2, 3 epoch 1
    for t in range(6):
        e, s = divmod(t, 2)
        want = [R.permute(s * B + i, N, 5, e) for i in range(B)]
        assert R.batch_indices(N, B, 5, t).tolist() == want


def _worst_cell_deviation(perms):
    """[n, B] permutations -> the largest |count - n/B| of the B x B position-by-row count matrix, in binomial sigmas."""
    n, B = perms.shape
    counts = np.zeros((B, B), dtype=np.int64)
    for j in range(B):
        counts[j] = np.bincount(perms[:, j], minlength=B)
    sigma = np.sqrt(n * (1.0 / B) * (1.0 - 1.0 / B))
    return float(np.abs(counts - n / B).max() / sigma)


@pytest.mark.parametrize("N", [8, 13])
def test_permutation_is_uniform(N):
    """Seed 1, epochs 0 .. 3999: every cell of the position-by-item count matrix within 5 binomial sigmas.  torch.randperm under a
    fixed generator is measured with the same statistic as the yardstick.  (N = 13 has bits = 4, a domain of 16: cycle walking.)"""
    n = 4000
    gen = torch.Generator().manual_seed(0)
    yard = np.stack([torch.randperm(N, generator=gen).numpy() for _ in range(n)])
    ours = R.permute_many(np.arange(N)[None, :], N, 1, np.arange(n)[:, None]).reshape(n, N)
    assert all(sorted(p.tolist()) == list(range(N)) for p in ours[:64])
    dev = _worst_cell_deviation(ours)
    print(f"N = {N} worst cell: ours {dev:.2f} sigma, torch.randperm {_worst_cell_deviation(yard):.2f} sigma")
    assert _worst_cell_deviation(yard) <= 5.0
    assert dev <= 5.0


# ---- the host API --------------------------------------------------------------------------------------------------------------------
def _store(**kw):
    from cavp_amd.store import DeviceStore
    kw = {"stage": (12, 20), "max_sources": 2, "max_channels": 2, "max_len": 50, "pcm_dtype": torch.int16, **kw}
    return DeviceStore(**kw)


def _item(h=5, w=7, srcs=((2, 9, 1),), dtype=np.int16, seed=0):
    rng = np.random.default_rng(seed)
    pcm = [(rng.integers(-100, 100, (c, n)).astype(dtype), r) for c, n, r in srcs]
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8), pcm


def test_append_and_constructor_fail_loudly():
    from cavp_amd._lib import CavpError
    from cavp_amd.store import BatchFeeder, DeviceStore
    st = _store()
    f, m, p = _item()
    with pytest.raises(CavpError, match="does not fit"):
        st.append(*_item(h=13))
    with pytest.raises(CavpError, match="does not fit"):
        st.append(*_item(w=21))
    with pytest.raises(CavpError, match="frame must be uint8"):
        st.append(f.astype(np.int32), m, p)
    with pytest.raises(CavpError, match="frame must be uint8"):
        st.append(f[:, :, :2], m, p)
    with pytest.raises(CavpError, match="mask must be uint8"):
        st.append(f, m[:-1], p)
    with pytest.raises(CavpError, match="pcm must be int16"):
        st.append(f, m, [(p[0][0].astype(np.float32), 0)])
    with pytest.raises(CavpError, match="outside"):
        st.append(*_item(srcs=((3, 9, 0),)))
    with pytest.raises(CavpError, match="outside"):
        st.append(*_item(srcs=((1, 51, 0),)))
    with pytest.raises(CavpError, match="max_sources"):
        st.append(*_item(srcs=((1, 5, 0),) * 3))
    with pytest.raises(CavpError, match="device tensor|numpy array"):
        st.append([[1]], m, p)
    assert len(st) == 0
    with pytest.raises(CavpError, match="empty"):
        st.freeze(upload=False)
    with pytest.raises(CavpError, match="pcm_dtype"):
        DeviceStore(stage=(4, 4), max_sources=1, max_channels=1, max_len=4, pcm_dtype=torch.float64)
    with pytest.raises(CavpError, match="stage"):
        DeviceStore(stage=(4, 1 << 15), max_sources=1, max_channels=1, max_len=4)
    for i in range(5):
        assert st.append(*_item(seed=i)) == i
    with pytest.raises(CavpError, match="no full batch"):
        BatchFeeder(st, batch=6)                        # spe == 0
    with pytest.raises(CavpError, match="no full batch"):
        BatchFeeder(st, batch=3, rank=1, world=3)       # ceil(5 / 3) = 2 per rank
    with pytest.raises(CavpError, match="rank"):
        BatchFeeder(st, batch=1, rank=2, world=2)
    assert BatchFeeder(st, batch=2).steps_per_epoch == 2
    assert BatchFeeder(st, batch=1, rank=1, world=2).steps_per_epoch == 3
    st.freeze(upload=False)
    with pytest.raises(CavpError, match="frozen"):
        st.append(f, m, p)
    with pytest.raises(CavpError, match="frozen"):
        st.freeze(upload=False)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_pack_is_back_to_back_and_item_reads_it_back(dtype):
    """No padding: the offsets are the running sums of the item sizes, and item(i) returns what was appended."""
    st = _store(pcm_dtype=torch.int16 if dtype is np.int16 else torch.float32)
    items = [_item(1, 1, (), dtype, 0), _item(5, 7, ((2, 9, 1),), dtype, 1), _item(12, 20, ((1, 50, 0), (2, 3, 2)), dtype, 2)]
    for it in items:
        st.append(*it)
    packed = st.pack()
    elem = np.dtype(dtype).itemsize
    assert packed["frame_off"].tolist() == [0, 3, 3 + 105] and packed["mask_off"].tolist() == [0, 1, 36]
    assert packed["pcm_off"].tolist() == [[0, 0], [0, 0], [18 * elem, 68 * elem]]
    assert packed["frames"].size == 3 + 105 + 720 and packed["pcm"].size == (18 + 50 + 6) * elem
    assert packed["n_src"].tolist() == [0, 1, 2] and packed["length"].tolist() == [[0, 0], [9, 0], [50, 3]]
    st.freeze(upload=False)
    assert st.nbytes == sum(v.nbytes for v in packed.values())
    for i, (f, m, p) in enumerate(items):
        gf, gm, gp = st.item(i)
        assert np.array_equal(gf, f) and np.array_equal(gm, m) and len(gp) == len(p)
        for (a, ra), (b, rb) in zip(gp, p):
            assert a.dtype == dtype and np.array_equal(a, b) and ra == rb


def test_restated_feed_writes_only_the_windows():
    items = [_item(1, 1, (), seed=0), _item(5, 7, ((2, 9, 1),), seed=1), _item(12, 20, ((1, 50, 0), (2, 3, 2)), seed=2)]
    ref = R.StoreRef(items, B=3)
    buf = {"frames": np.full((3, 12, 20, 3), 0xA5, np.uint8), "masks": np.full((3, 12, 20), 0xA5, np.uint8),
           "pcm": np.full((3, 2, 2, 50), 0x5A5A, np.int16), "sizes": np.zeros((3, 2), np.int32), "index": np.zeros(3, np.int32),
           "length": np.full((3, 2), -1, np.int32), "rate_idx": np.full((3, 2), -1, np.int32), "n_ch": np.full((3, 2), -1, np.int32)}
    ref.feed(buf, index=[1, 7, 0])
    assert ref.bad == 1 and ref.t == 1 and buf["index"].tolist() == [1, 0, 0]
    assert np.array_equal(buf["frames"][0, :5, :7], items[1][0]) and (buf["frames"][0, 5:] == 0xA5).all() and (buf["frames"][0, :, 7:] == 0xA5).all()
    assert buf["length"].tolist() == [[9, 0], [0, 0], [0, 0]] and buf["rate_idx"].tolist() == [[1, -1], [-1, -1], [-1, -1]]
    assert (buf["pcm"][0, 0, :, 9:] == 0x5A5A).all() and (buf["pcm"][1:] == 0x5A5A).all()
