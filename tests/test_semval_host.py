"""CPU checks of cavp_amd.metrics.SemanticValidation: the exports, the two entry points in the built library, the argument checks,
the host reduction of results(), and the CPU restatement tests/_semval_ref.py against tests/golden/semval.npz
(tools/make_golden_semval.py ran the reference's calc_color_miou_fscore / calc_color_miou / calc_binary_miou).

Bounds: the integer counts are compared exactly; ious / fscores / cls_count bit for bit (per class the restatement performs the
reference's float32 operations in the reference's order); frame_miou and the binary value within 4 float32 ulp, because the
reference's torch.sum does not add in ascending order and a sum of at most 5 positive terms differs by at most 4 roundings."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cavp_amd import _lib, ops
from cavp_amd import metrics as MT
from cavp_amd._lib import CavpError

from tests import _semval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "semval.npz")
CASES = {"vec": (5, (24, 28)), "sca": (3, (7, 9))}
B, T = 2, 3


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def assert_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def assert_ulp(got, want, ulp=4):
    got, want = np.atleast_1d(np.asarray(got, np.float32)), np.atleast_1d(np.asarray(want, np.float32))
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) <= ulp * np.spacing(np.abs(want[ok])).astype(np.float64)).all(), \
        (got, want)


def test_exported():
    for name in ("SemanticValidation", "calc_color_miou_fscore", "calc_color_miou", "calc_binary_miou"):
        assert name in MT.__all__ and callable(getattr(MT, name))
    assert callable(ops.semval_update)


def test_symbols_and_abi():
    lib = _lib.load()
    assert _lib.ABI_VERSION == lib.cavp_abi_version() == 16
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cavp_semval_frame_counts", "cavp_semval_combine"):
        assert name in _lib.PROTOTYPES and getattr(raw, name) is not None
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cavp_hip.h")).read()
    assert "int cavp_semval_frame_counts(" in header and "int cavp_semval_combine(" in header
    assert len(_lib.PROTOTYPES["cavp_semval_frame_counts"][1]) == 13 and len(_lib.PROTOTYPES["cavp_semval_combine"][1]) == 12


def test_fixture_holds_the_required_frames(z):
    for name, (K, hw) in CASES.items():
        logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
        assert logits.shape == (B, T, K) + hw and labels.shape == (B, T) + hw and labels.dtype == np.int64
        top = np.sort(logits, axis=2)
        assert (top[:, :, -1] - top[:, :, -2] > 1e-3).all()                       # no argmax ties
        amax = logits.argmax(2)
        values = set(np.unique(labels).tolist())
        assert {255, -1, K + 2} <= values and K + 2 != 255
        assert (labels[0, 1] == 0).all() and (amax[0, 1] == 0).all()              # an all-background frame
        assert (amax != K - 1).all() and (labels == K - 1).any()                  # a class that is never predicted
        assert (labels[1, 2] == 0).all() and (amax[1, 2] != 0).any()              # an empty foreground
        assert np.isnan(z[f"{name}_one_vid"]).sum() == 0
        for v in list(z[f"{name}_one_vid"]) + [float(z[f"{name}_one_binary"])]:
            assert v >= 1e-5
    assert (24 * 28) % 4 == 0 and (7 * 9) % 4 != 0


@pytest.mark.parametrize("name", list(CASES))
def test_ref_reproduces_fixture(z, name):
    K, (H, W) = CASES[name]
    logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
    flat = logits.reshape(B * T, K, H, W)
    one = R.call(flat, labels, None, K)
    np.testing.assert_array_equal(one["counts"], z[f"{name}_counts"])
    runs = {"one": one, "a": R.call(logits[0], labels[0], None, K), "b": R.call(logits[1], labels[1], None, K)}
    for run, got in runs.items():
        n = len(z[f"{name}_{run}_vid"])
        print(name, run, "frame_miou", got["frame_miou"], z[f"{name}_{run}_vid"], "binary", got["binary"] / np.float32(n),
              z[f"{name}_{run}_binary"])
        assert_bits(got["ious"], z[f"{name}_{run}_ious"])
        assert_bits(got["fscores"], z[f"{name}_{run}_fscores"])
        assert_bits(got["cls_count"], z[f"{name}_{run}_cls_count"])
        assert_bits(got["ious"], z[f"{name}_{run}_ious2"])                        # calc_color_miou
        assert_bits(got["cls_count"], z[f"{name}_{run}_cls2"])
        assert_ulp(got["frame_miou"], z[f"{name}_{run}_vid"])
        assert_ulp(got["binary"] / np.float32(n), z[f"{name}_{run}_binary"])
        assert got["frames"] == n and got["bad_mask"] == 0 and got["bad_count"] == 0
    acc = R.Accumulator(K)                                                        # two calls, added as the driver adds them
    acc.update(logits[0], labels[0])
    acc.update(logits[1], labels[1])
    for i, key in enumerate(("ious", "fscores", "cls_count")):
        assert_bits(acc.accumulators()[i], z[f"{name}_two_{key}"])
    assert acc.frames == B * T


def test_ref_count_and_quirks():
    """count below T skips frames; a label >= K counts in pred only, a negative one nowhere; a mask byte >= K sets no class counter."""
    K = 3
    labels = np.array([[[[0, 1, 2, 255], [-1, 7, 1, 1]]], [[[0, 0, 0, 0], [0, 0, 0, 0]]]], dtype=np.int64)       # [2, 1, 2, 4]
    mask = np.array([[[0, 1, 1, 2], [2, 1, 1, 0]], [[9, 9, 9, 9], [9, 9, 9, 9]]], dtype=np.uint8)
    r = R.call(mask, labels, [1, 0], K)
    assert r["frames"] == 1 and r["bad_mask"] == 0 and not r["counts"][1].any() and r["frame_miou"][1] == -1
    inter, pred, lab, binary = np.split(r["counts"][0], [K, 2 * K, 3 * K])
    assert inter.tolist() == [1, 2, 0] and pred.tolist() == [2, 4, 1] and lab.tolist() == [1, 3, 1]
    assert binary.tolist() == [6, 7, 1, 7]
    r = R.call(mask, labels, [5, -2], K)
    assert r["bad_count"] == 2 and r["frames"] == 1
    r = R.call(mask, labels, None, K)
    assert r["bad_mask"] == 8 and not r["counts"][1][:3 * K].any() and r["counts"][1][3 * K:].tolist() == [0, 8, 0, 0]


def test_before_any_update():
    sv = MT.SemanticValidation(num_classes=5)
    assert sv.accumulators().shape == (3, 5) and float(sv.accumulators().sum()) == 0 and sv.frames() == 0
    with pytest.raises(CavpError, match="no frame"):
        sv.results()
    with pytest.raises(CavpError):
        sv.check()
    with pytest.raises(CavpError):
        sv.last_call()
    sv.reset()


def test_bad_constructor_arguments_raise():
    for kw in (dict(num_classes=1), dict(num_classes=0), dict(num_classes=MT.MAX_CLASSES + 1), dict(num_classes=5, max_frames=0),
               dict(num_classes=5, max_frames=65536)):
        with pytest.raises(CavpError):
            MT.SemanticValidation(**kw)
    MT.SemanticValidation(num_classes=2)
    MT.SemanticValidation(num_classes=MT.MAX_CLASSES, max_frames=320)


def test_cpu_tensors_raise():
    sv = MT.SemanticValidation(num_classes=3, device="cuda:0")
    lab = torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    with pytest.raises(CavpError, match="CPU"):
        sv.update(torch.zeros(4, 3, 8, 8), lab)
    with pytest.raises(CavpError, match="CPU"):
        sv.update(torch.zeros(4, 8, 8, dtype=torch.uint8), lab, torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(CavpError, match="CPU"):
        sv.update_lowres(torch.zeros(4, 2, 2, 3), lab)
    for fn in (MT.calc_color_miou_fscore, MT.calc_color_miou, MT.calc_binary_miou):
        with pytest.raises(CavpError, match="CPU"):
            fn(torch.zeros(4, 3, 8, 8), lab[0])


def test_malformed_arguments_raise():
    sv = MT.SemanticValidation(num_classes=3, max_frames=4, device="cuda:0")
    lab = torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    logits = torch.zeros(4, 3, 8, 8)
    cnt = torch.tensor([1, 2], dtype=torch.int32)
    bad = [
        (logits, lab.int(), None),                                        # labels not int64
        (logits, lab[0, 0], None),                                        # labels 2-d
        (logits, lab.flatten(0, 1), cnt),                                 # count with 3-d labels
        (logits[:3], lab, None),                                          # N != B * T
        (logits[:, :, :, :7], lab, None),                                 # H x W differ
        (logits.double(), lab, None),                                     # logits dtype
        (torch.zeros(4, 2, 8, 8), lab, None),                             # C < K
        (torch.zeros(4, 4, 8, 8), lab, None),                             # C > K
        (torch.zeros(4, 3, 8), lab, None),                                # logits 3-d
        (torch.zeros(4, 8, 9, dtype=torch.uint8), lab, None),             # mask shape
        (logits, lab, cnt.float()),                                       # count dtype
        (logits, lab, cnt[:1]),                                           # count shape
        (logits, lab, [1, 2]),                                            # count no tensor
        (torch.zeros(6, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.int64), None),   # more than max_frames frames
        (logits, lab.transpose(2, 3), None),                              # labels not dense
        (logits.transpose(2, 3), lab, None),                              # logits not dense
    ]
    for pred, labels, count in bad:
        with pytest.raises(CavpError) as e:
            sv.update(pred, labels, count)
        assert "CPU" not in str(e.value), (getattr(pred, "shape", None), labels.shape)   # refused for its own reason
    lo = torch.zeros(4, 2, 2, 3)
    bad_lo = [
        dict(lo=lo[:3], labels=lab),                                      # N != B * T
        dict(lo=lo.double(), labels=lab),                                 # dtype
        dict(lo=lo, labels=lab, input_shape=(8, 9)),                      # input_shape differs from the labels'
        dict(lo=torch.zeros(4, 2, 2, 4), labels=lab),                     # C != K
        dict(lo=lo, labels=lab.flatten(0, 1), count=cnt),                 # count with 3-d labels
    ]
    for kw in bad_lo:
        with pytest.raises(CavpError) as e:
            sv.update_lowres(**kw)
        assert "CPU" not in str(e.value), kw
    with pytest.raises(CavpError, match="eps"):
        MT.calc_binary_miou(logits, lab[0], eps=1e-6)


def test_results_on_hand_made_accumulators():
    """The driver's reduction: per-class quotients with NaN -> 0 (a class that never occurred), means over ALL K classes."""
    ious = np.array([2.5, 0.0, 1.25, 0.75], np.float32)
    fscores = np.array([2.75, 0.0, 0.5, 1.0], np.float32)
    cls_count = np.array([3.0, 0.0, 2.0, 7.0], np.float32)
    got = MT.SemanticValidation._finish(torch.from_numpy(ious.copy()), torch.from_numpy(fscores.copy()), torch.from_numpy(cls_count.copy()),
                                        torch.tensor(4.5), 7)
    ref = R.results(ious, fscores, cls_count, np.float32(4.5), 7)
    assert_bits(got["miou_pc"].numpy(), ref["miou_pc"])
    assert_bits(got["fscore_pc"].numpy(), ref["fscore_pc"])
    assert got["miou_pc"][1] == 0 and got["fscore_pc"][1] == 0
    assert_bits(got["cls_count"].numpy(), cls_count)
    miou, fscore = torch.from_numpy(ref["miou_pc"]).mean(), torch.from_numpy(ref["fscore_pc"]).mean()
    assert got["miou"] == miou.item() and got["fscore"] == fscore.item() and got["jf"] == ((miou + fscore) / 2).item()
    assert abs(got["miou"] - (2.5 / 3 + 0.625 + 0.75 / 7) / 4) < 1e-6               # over all 4 classes, the empty one included
    assert got["binary_miou"] == float(ref["binary_miou"]) == float(np.float32(4.5) / np.float32(7))
    with pytest.raises(CavpError, match="no frame"):
        MT.SemanticValidation._finish(torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.tensor(0.0), 0)
