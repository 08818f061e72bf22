"""Device DropPath sampler, host side (cavp_amd/droppath.py): the entry point and its prototype, the opt-in's argument
checks, and the numpy restatement of the draw rule (tests/_droppath_ref.py) on its own - values, offsets, and the kept fraction of
every branch of PVTv2-B5's keep table."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import _droppath_ref as R

SEED = 0          # the committed seed of the statistics below: passes with the reference on the CPU (checked before committing)


def test_entry_point_and_abi():
    from cavp_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 16 == lib.cavp_abi_version()
    assert hasattr(lib, "cavp_drop_path_draw")
    res, args = _lib.PROTOTYPES["cavp_drop_path_draw"]
    assert res is ctypes.c_int32 and len(args) == 7
    # rejected before any launch: null pointers, n < 1, B < 1, n * B > 2^20
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad_arg, unsupported = -1, -2
    assert lib.cavp_drop_path_draw(None, p, p, 1, 1, p, None) == bad_arg
    assert lib.cavp_drop_path_draw(p, None, p, 1, 1, p, None) == bad_arg
    assert lib.cavp_drop_path_draw(p, p, None, 1, 1, p, None) == bad_arg
    assert lib.cavp_drop_path_draw(p, p, p, 1, 1, None, None) == bad_arg
    assert lib.cavp_drop_path_draw(p, p, p, 0, 1, p, None) == bad_arg
    assert lib.cavp_drop_path_draw(p, p, p, 1, 0, p, None) == bad_arg
    assert lib.cavp_drop_path_draw(p, p, p, 1025, 1024, p, None) == unsupported
    assert lib.cavp_drop_path_draw(p, p, p, 1 << 20, 1 << 20, p, None) == unsupported


def test_use_device_drop_path_is_pvt_only():
    from cavp_amd._lib import CavpError
    from cavp_amd.cavp_model import CAVP
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, False, False], audio_backbone="vgg",
                                 num_classes=2, batch_size=2, local_rank="cpu")
    m = CAVP(50, None, num_classes=2, args=args)
    with pytest.raises(CavpError):
        m.use_device_drop_path(seed=0)
    with pytest.raises(CavpError):
        m.use_device_drop_path(None)


def test_sampler_constructor_touches_no_device(monkeypatch):
    from cavp_amd.droppath import DropPathSampler

    def boom(*a, **k):
        raise AssertionError("the constructor touched the device")
    for name in ("zeros", "empty", "tensor"):
        monkeypatch.setattr(torch, name, boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    dp = DropPathSampler(seed=5)
    assert dp._state is None and dp._seed == 5
    dp.manual_seed(-3)                       # still host only
    assert dp._state is None and dp._seed == -3
    dp.manual_seed((1 << 64) - 1)            # 64-bit two's complement, as FrameAugment's
    assert dp._seed == -1


def test_reference_philox_known_answers_and_vector_form():
    # Random123's known-answer vectors for philox4x32-10 (first output word)
    assert R.philox_word0(0, 0, 0, 0, 0, 0) == 0x6627E8D5
    assert R.philox_word0(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == 0x408F276D
    assert R.philox_word0(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == 0xD16CFE09
    c0, c1 = np.arange(7)[None, :], np.arange(5)[:, None]
    for c2, c3, k0, k1 in ((0, 0, 0, 0), (0xFFFFFFFF, 1, 0x9ABCDEF0, 0x12345678), (3, 0, 0xFFFFFFFF, 0xFFFFFFFF)):
        many = R.philox_word0_many(c0, c1, c2, c3, k0, k1)
        assert many.shape == (5, 7)
        for k in range(5):
            for b in range(7):
                assert int(many[k, b]) == R.philox_word0(b, k, c2, c3, k0, k1)
    u = R.u01(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


@pytest.fixture(scope="module")
def b5_tables():
    from cavp_amd.pvt import pvt_v2_b5
    bb = pvt_v2_b5()
    probs = [blk.drop_prob for i in range(4) for blk in getattr(bb, f"block{i + 1}") for _ in range(2)]
    assert len(probs) == 2 * sum(bb.depths) and probs[0] == 0.0 and probs[1] == 0.0 and all(p > 0 for p in probs[2:])
    keep, inv = R.keep_tables(probs)
    assert keep.shape == inv.shape == (sum(1 for p in probs if p > 0),)
    return keep, inv


def test_reference_values_and_offsets(b5_tables):
    keep, inv = b5_tables
    n, B = keep.shape[0], 64
    a = R.ref_scales(SEED, 0, keep, inv, B)
    assert a.dtype == np.float32 and a.shape == (n, B)
    # 0 or inv_keep[k], exactly
    assert np.all((a.view(np.int32) == 0) | (a.view(np.int32) == np.broadcast_to(inv[:, None], a.shape).view(np.int32)))
    assert (a == 0).any() and (a != 0).any()
    assert np.array_equal(a, R.ref_scales(SEED, 0, keep, inv, B))                 # a pure function
    b = R.ref_scales(SEED, 1, keep, inv, B)
    assert not np.array_equal(a, b)                                               # rows at different offsets differ
    assert not np.array_equal(a, R.ref_scales(SEED + 1, 0, keep, inv, B))
    assert not np.array_equal(a, R.ref_scales(SEED, 1 << 32, keep, inv, B))       # the high offset word counts
    assert not np.array_equal(a, R.ref_scales(SEED + (1 << 32), 0, keep, inv, B))  # and the high seed word
    assert np.array_equal(R.ref_scales(-1, 0, keep, inv, B), R.ref_scales((1 << 64) - 1, 0, keep, inv, B))   # two's complement
    # a sample's draw does not depend on the batch size
    assert np.array_equal(R.ref_scales(SEED, 5, keep, inv, 3), R.ref_scales(SEED, 5, keep, inv, B)[:, :3])
    # keep = 1 always survives, and the limit of the rule: u < 1, so a branch with keep -> 0 never does
    one = R.ref_scales(SEED, 0, np.ones(4, np.float32), np.ones(4, np.float32), B)
    assert np.all(one == 1.0)


def test_reference_kept_fraction_of_every_branch(b5_tables):
    """PVTv2-B5's keep table, B = 64, offsets 0 .. 255: N = 16384 draws per branch; the kept fraction of every branch within
    4 sigma = 4 sqrt(keep (1 - keep) / N) of keep[k]."""
    keep, inv = b5_tables
    B, offsets = 64, 256
    N = B * offsets
    kept = np.zeros(keep.shape[0], dtype=np.int64)
    for o in range(offsets):
        kept += (R.ref_scales(SEED, o, keep, inv, B) != 0).sum(axis=1)
    frac = kept / N
    k64 = keep.astype(np.float64)
    bound = 4.0 * np.sqrt(k64 * (1.0 - k64) / N)
    worst = float(np.max(np.abs(frac - k64) / bound))
    print(f"device DropPath reference, seed {SEED}: worst |fraction - keep| / (4 sigma) = {worst:.3f} over {keep.shape[0]} branches")
    assert np.all(np.abs(frac - k64) <= bound), worst
