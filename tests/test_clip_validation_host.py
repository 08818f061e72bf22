"""CPU checks of cavp_amd.metrics.ClipValidation: the export, the two entry points in the built library, the argument checks, and
the CPU restatement tests/_clipval_ref.py against tests/golden/clip_validation.npz (tools/make_golden_clipval.py ran the reference's
MIoU / ForegroundDetect through the AVSS validation loop), including that the fixture tells mutated predicates apart."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cavp_amd import _lib
from cavp_amd import metrics as MT
from cavp_amd._lib import CavpError

from tests import _clipval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_validation.npz")
CASES = ("a", "b")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _case(z, name):
    lq, labels = z[f"{name}_logits_q"], z[f"{name}_labels"]
    logits = torch.from_numpy(lq.astype(np.float32) / 8).flatten(0, 1)
    return logits, labels, z[f"{name}_mask_num"], lq.shape[2]


def test_exported():
    assert "ClipValidation" in MT.__all__ and callable(MT.ClipValidation)


def test_symbols_and_abi():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 16 == lib.cavp_abi_version()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cavp_clipval_frame_counts", "cavp_clipval_combine"):
        assert name in _lib.PROTOTYPES and getattr(raw, name) is not None


def test_fixture_holds_the_required_frames(z):
    lab = z["a_labels"]
    qualifying = lambda f: int((np.unique(np.where(f < 0, 255, f), return_counts=True)[1] > 100).sum())   # noqa: E731
    n = [[qualifying(f) for f in clip] for clip in lab]
    assert 2 in n[0] and 3 in n[0]
    counts = np.concatenate([np.unique(f, return_counts=True)[1] for f in lab[0]])
    assert 100 in counts and 101 in counts
    assert any(qualifying(f) == 3 and (f == 255).sum() > 100 for f in lab[0])
    mask_num, T = z["a_mask_num"], lab.shape[1]
    assert 0 in mask_num and T in mask_num


@pytest.mark.parametrize("name", CASES)
def test_ref_reproduces_fixture(z, name):
    logits, labels, mask_num, K = _case(z, name)
    for pred in (logits, logits.argmax(1).to(torch.uint8)):
        got = R.clip_validation(pred, labels, mask_num, K)
        np.testing.assert_array_equal(got["counts"], z[f"{name}_M"])
        assert got["frames"] == tuple(z[f"{name}_frames"]) and got["bad"] == [0, 0, 0]
        assert R.results(got["counts"]) == z[f"{name}_results"].tolist()


@pytest.mark.parametrize("mutation", ["at_least", "skip_ignore", "lump_large"])
def test_fixture_tells_mutations_apart(z, mutation):
    logits, labels, mask_num, K = _case(z, "a")
    got = R.clip_validation(logits, labels, mask_num, K, **{mutation: True})
    np.testing.assert_array_equal(got["counts"][0], z["a_M"][0])          # ALL does not depend on the predicate
    assert not np.array_equal(got["counts"][1], z["a_M"][1])
    assert got["frames"] != tuple(z["a_frames"])
    assert R.results(got["counts"]) != z["a_results"].tolist()


def test_accessors_read_adopted_counts(z):
    M = torch.from_numpy(z["a_M"].copy())
    m, f = MT.MIoU(8, 255, 0)._adopt(M[0]), MT.ForegroundDetect(8)._adopt(M[0])
    assert [float(v) for v in MT.get_performance(m, f)] == z["a_results"][:5].tolist()
    M[0] += M[1]                                                           # no copy: the next read sees the owner's update
    assert int(m.counts().sum()) == int(M[0].sum())
    with pytest.raises(CavpError):
        MT.MIoU(8, 255, 0)._adopt(torch.zeros(7, dtype=torch.int64))


def test_before_any_update():
    cv = MT.ClipValidation(num_classes=8)
    assert cv.frames() == (0, 0) and cv.counts().shape == (2, 9, 8) and int(cv.counts().sum()) == 0
    assert cv.results()[0][:2] == (0.0, 0.0)
    with pytest.raises(CavpError):
        cv.check()


def test_bad_constructor_arguments_raise():
    for kw in (dict(num_classes=0), dict(num_classes=4097), dict(num_classes=8, ignore_index=256),
               dict(num_classes=8, ignore_index=-1), dict(num_classes=8, ignore_index=None), dict(num_classes=8, max_frames=0),
               dict(num_classes=8, min_count=-1), dict(num_classes=8, min_values=-1), dict(num_classes=4096, max_frames=320)):
        with pytest.raises(CavpError):
            MT.ClipValidation(**kw)


def test_cpu_tensors_raise():
    cv = MT.ClipValidation(num_classes=3, device="cuda:0")
    lab = torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    with pytest.raises(CavpError, match="CPU"):
        cv.update(torch.zeros(4, 8, 8, dtype=torch.uint8), lab)
    with pytest.raises(CavpError, match="CPU"):
        cv.update(torch.zeros(4, 3, 8, 8), lab, torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(CavpError):
        MT.ClipValidation(num_classes=3, device="cpu").update(torch.zeros(4, 8, 8, dtype=torch.uint8), lab)


def test_malformed_arguments_raise():
    cv = MT.ClipValidation(num_classes=3, max_frames=4, device="cuda:0")
    lab = torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    mask, logits = torch.zeros(4, 8, 8, dtype=torch.uint8), torch.zeros(4, 3, 8, 8)
    cnt = torch.tensor([1, 2], dtype=torch.int32)
    bad = [
        (mask, lab.int(), None),                                          # labels not int64
        (mask, lab[0, 0], None),                                          # labels 2-d
        (mask, lab.flatten(0, 1), cnt),                                   # count without [B, T, H, W] labels
        (mask[:3], lab, None),                                            # N != B * T
        (torch.zeros(4, 8, 9, dtype=torch.uint8), lab, None),             # H x W differ
        (mask.long(), lab, None),                                         # mask dtype
        (logits.double(), lab, None),                                     # logits dtype
        (logits[:, :, :, :7], lab, None),                                 # logits H x W differ
        (torch.zeros(4, 4, 8, 8), lab, None),                             # more channels than classes
        (torch.zeros(4, 3, 8), lab, None),                                # logits 3-d
        (mask, lab, cnt.float()),                                         # count dtype
        (mask, lab, cnt[:1]),                                             # count shape
        (mask, lab, [1, 2]),                                              # count no tensor
        (torch.zeros(6, 8, 8, dtype=torch.uint8), torch.zeros(2, 3, 8, 8, dtype=torch.int64), None),   # N > max_frames
        (mask, lab.transpose(2, 3), None),                                # labels not dense
    ]
    for pred, labels, count in bad:
        with pytest.raises(CavpError) as e:
            cv.update(pred, labels, count)
        assert "CPU" not in str(e.value), (pred.shape, labels.shape)      # refused for its own reason, before the device check
