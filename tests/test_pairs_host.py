"""CPU-side checks of the pair builder (cavp_amd/pairs.py, csrc/pairs.hip): the library exports the four entry points and the
header, the exports and the ctypes table agree; the numpy restatement (tests/_pairs_ref.py) equals what the reference's own
SoundBank + overwrite_miss_match recorded in tests/golden/pairs.npz; the public entry fails loudly; the overwrite-count table
is Python's; the restated permutation is uniform."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _pairs_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cavp_pairs_plan", "cavp_pairs_gather", "cavp_pairs_bank_update", "cavp_pairs_labels")


def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "pairs.npz"))


def test_library_exports_the_pair_entry_points():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == _lib.load().cavp_abi_version()


def test_header_and_ctypes_table_agree():
    from cavp_amd import _lib
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


def _replay(ref, g, s):
    rank = R.rank_from_draw(g["if_match_shuffle"][s], g["ow_draw"][s]) if g["overwrite"][s] else None
    return ref(g["waveform"][s], g["pix_label"][s], g["img_label"][s], bool(g["overwrite"][s]), perm=g["perm"][s], ow_rank=rank)


def assert_step_equals_golden(out, bank, g, s):
    """`out`: the builder's / the restatement's outputs as numpy arrays; bank: [K, S, A] in logical order after the step."""
    B = g["waveform"].shape[1]
    assert np.array_equal(out["perm"], g["perm"][s])
    assert np.array_equal(out["if_match"].astype(bool), g["if_match"][s])
    assert np.array_equal(out["img_label_shuffle"], g["img_label_shuffle"][s])
    mod = np.where(out["source"] < 0, ~out["source"], -1)
    assert np.array_equal(mod, g["mod_idx_map"][s])
    assert np.array_equal(out["source"][mod < 0], g["perm"][s][mod < 0])
    assert np.array_equal(out["waveforms"][:B], g["waveform"][s])
    assert np.array_equal(out["waveforms"][B:], g["shuffle_audio"][s])
    assert np.array_equal(out["label_shuffle"], g["shuffle_pix_label"][s])
    assert np.array_equal(bank, g["bank"][s])


def test_restatement_equals_reference_fixture():
    g = golden()
    B, K, S, A, H, W, steps = (int(v) for v in g["config"])
    ref = R.PairsRef(K, S, A, float(g["ow_rate"]))
    seen_ow = 0
    for s in range(steps):
        out = _replay(ref, g, s)
        assert out["n_false"] == int(g["n_false"][s])
        assert_step_equals_golden(out, ref.bank, g, s)
        seen_ow += int((out["source"] < 0).sum())
    assert seen_ow >= 8       # the fixture does exercise the overwrite


def test_fixture_shows_the_three_cases():
    """An empty (all-zero) slot 0 handed out, a ring wrap, and an overwritten class pushed in the same step."""
    g = golden()
    B, K, S, A, H, W, steps = (int(v) for v in g["config"])
    pushes = np.zeros(K, dtype=int)
    zero_slot = hazard = False
    for s in range(steps):
        img = g["img_label"][s]
        single = np.where((img[:, 1:] != 0).sum(1) == 1, (img[:, 1:] != 0).argmax(1) + 1, -1)
        for i in np.flatnonzero(g["mod_idx_map"][s] >= 0):
            c = g["mod_idx_map"][s][i]
            zero_slot |= pushes[c] < S and not g["shuffle_audio"][s][i].any()
            hazard |= pushes[c] >= S and c in single
        for c in single[single >= 0]:
            pushes[c] += 1
    assert zero_slot and hazard and (pushes > S).any()


def _cpu_inputs(B=4, C=1, K=6, A=64, hw=8):
    return torch.zeros(B, C, A), torch.zeros(B, hw, hw, dtype=torch.int64), torch.zeros(B, K, dtype=torch.int64)


def test_pair_builder_fails_loudly():
    from cavp_amd._lib import CavpError
    from cavp_amd.pairs import PairBuilder
    pb = PairBuilder(num_classes=6, bank_slots=4, wave_len=64, ow_rate=0.5, max_batch=8)
    wav, pix, img = _cpu_inputs()
    with pytest.raises(CavpError, match="CPU tensor"):
        pb(wav, pix, img, True)
    with pytest.raises(CavpError, match="stereo"):
        pb(_cpu_inputs(C=2)[0], pix, img, True)
    with pytest.raises(CavpError, match="max_batch"):
        pb(*_cpu_inputs(B=9), True)
    with pytest.raises(CavpError, match="float32"):
        pb(wav.double(), pix, img, True)
    with pytest.raises(CavpError, match="pix_label"):
        pb(wav, pix.int(), img, True)
    with pytest.raises(CavpError, match="img_label"):
        pb(wav, pix, img.int(), True)
    with pytest.raises(CavpError, match="perm"):
        pb(wav, pix, img, True, perm=torch.arange(4))
    with pytest.raises(CavpError, match="ow_rank"):
        pb(wav, pix, img, True, ow_rank=torch.arange(4))
    with pytest.raises(CavpError):
        PairBuilder(num_classes=6, bank_slots=4, wave_len=64, ow_rate=0.5, max_batch=1025)
    with pytest.raises(CavpError):
        PairBuilder(num_classes=257, bank_slots=4, wave_len=64, ow_rate=0.5)
    with pytest.raises(CavpError):
        pb.last_plan()


@pytest.mark.parametrize("rate", [0.3, 0.5, 0.7, 1.0])
def test_overwrite_count_table_is_pythons(rate):
    from cavp_amd.pairs import PairBuilder
    pb = PairBuilder(num_classes=6, bank_slots=4, wave_len=64, ow_rate=rate, max_batch=1024)
    assert pb.ow_table_host.dtype == np.int32 and pb.ow_table_host.shape == (1025,)
    assert pb.ow_table_host.tolist() == [int(n * rate) for n in range(1025)]
    assert R.ow_table(1024, rate).tolist() == pb.ow_table_host.tolist()


def _worst_cell_deviation(perms):
    """[n, B] permutations -> the largest |count - n/B| of the B x B position-by-row count matrix, in binomial sigmas."""
    n, B = perms.shape
    counts = np.zeros((B, B), dtype=np.int64)
    for j in range(B):
        counts[j] = np.bincount(perms[:, j], minlength=B)
    sigma = np.sqrt(n * (1.0 / B) * (1.0 - 1.0 / B))
    return float(np.abs(counts - n / B).max() / sigma)


def test_restated_permutation_is_uniform():
    """B = 8, 4000 consecutive offsets: every cell of the 8 x 8 count matrix within 5 sigma of the binomial (500 +- 5 * sqrt(500 *
    7 / 8)).  torch.randperm under a fixed generator is measured with the same statistic as the yardstick."""
    B, n = 8, 4000
    gen = torch.Generator().manual_seed(0)
    yard = np.stack([torch.randperm(B, generator=gen).numpy() for _ in range(n)])
    assert _worst_cell_deviation(yard) <= 5.0
    ours = np.stack([R.draw_perm(B, seed=0, offset=o) for o in range(n)])
    assert all(sorted(p.tolist()) == list(range(B)) for p in ours[:64])
    dev = _worst_cell_deviation(ours)
    print(f"worst cell: ours {dev:.2f} sigma, torch.randperm {_worst_cell_deviation(yard):.2f} sigma")
    assert dev <= 5.0
