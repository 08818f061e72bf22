"""CPU checks of cavp_amd.metrics.VideoValidation: the export, the two entry points in the built library, the argument checks, and
the CPU restatement tests/_videoval_ref.py against tests/golden/videoval.npz (tools/make_golden_videoval.py ran the reference's
mask_iou / Eval_Fmeasure / MIoU / ForegroundDetect / AverageMeter through the AVSBench object validation loop)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cavp_amd import _lib, ops
from cavp_amd import metrics as MT
from cavp_amd._lib import CavpError

from tests import _videoval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "videoval.npz")
CASES = ("vec", "sca")
T = 5
BOUND = (T + 8) * 2.0 ** -24      # each score is in [0, 1] and the result of at most T + 8 float32 roundings of positive terms


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def test_exported():
    assert "VideoValidation" in MT.__all__ and callable(MT.VideoValidation)
    assert callable(ops.videoval_frame_stats) and callable(ops.videoval_combine)


def test_symbols_and_abi():
    lib = _lib.load()
    assert _lib.ABI_VERSION == lib.cavp_abi_version()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cavp_videoval_frame_stats", "cavp_videoval_combine"):
        assert name in _lib.PROTOTYPES and getattr(raw, name) is not None
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cavp_hip.h")).read()
    assert "int cavp_videoval_frame_stats(" in header and "int cavp_videoval_combine(" in header
    assert f"#define CAVP_VIDEOVAL_MAX_THRESHOLDS {ops.VIDEOVAL_MAX_THRESHOLDS}\n" in header


def test_fixture_holds_the_required_frames(z):
    th = R.thresholds().astype(np.float64)
    for name, hw in zip(CASES, ((24, 28), (7, 9))):
        logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
        assert logits.shape == (4, T, 2) + hw and labels.shape == (4, T) + hw
        gt = labels.reshape(4, T, -1).sum(-1)
        assert (gt[2] == 0).all() and gt[1, 3] == 0 and (np.delete(gt[1], 3) > 0).all()
        assert z[f"{name}_F"][2] == 0.0 and z[f"{name}_J"][2] > 0.0
        d = logits.astype(np.float64)
        p = 1.0 / (1.0 + np.exp(d[:, :, 0] - d[:, :, 1]))                  # the float64 softmax of channel 1, C = 2
        assert np.abs(p[..., None] - th).min() >= 0.99e-5                   # the generator's margin condition on the inputs
    assert (24 * 28) % 4 == 0 and (7 * 9) % 4 != 0


@pytest.mark.parametrize("name", CASES)
def test_ref_reproduces_fixture(z, name):
    logits, labels = z[f"{name}_logits"], z[f"{name}_labels"]
    got = R.video_validation(logits.reshape((-1,) + logits.shape[2:]), labels, None, 2)
    np.testing.assert_array_equal(got["stats"], z[f"{name}_stats"])
    np.testing.assert_array_equal(got["hist"], z[f"{name}_hist"])
    np.testing.assert_array_equal(got["M"], z[f"{name}_M"])
    assert got["state"] == [0, 0, 0, 0, 4, 0, 0, 0]
    for k in range(4):
        print(name, k, "J", got["J"][k], z[f"{name}_J"][k], "F", got["F"][k], z[f"{name}_F"][k])
    np.testing.assert_allclose(np.array(got["J"], np.float64), z[f"{name}_J"].astype(np.float64), rtol=0, atol=BOUND)
    np.testing.assert_allclose(np.array(got["F"], np.float64), z[f"{name}_F"], rtol=0, atol=BOUND)
    m = R.means(got["J"], got["F"])
    np.testing.assert_allclose(m, z[f"{name}_means"], rtol=0, atol=BOUND)
    assert [float(np.round(v, 4)) for v in m] == z[f"{name}_rounded"].tolist()
    assert R.performance(got["M"]) == z[f"{name}_perf"].tolist()


def test_ref_count_and_slots(z):
    """count below T is the loop over the first count[b] frames; a video without frames takes no slot; slots beyond max_videos drop."""
    logits, labels = z["sca_logits"], z["sca_labels"]
    flat = logits.reshape((-1,) + logits.shape[2:])
    got = R.video_validation(flat, labels, [T, 2, 0, 9], 2, max_videos=2)
    assert got["state"] == [0, 0, 1, 1, 3, 0, 0, 0] and len(got["J"]) == 2
    whole = R.video_validation(flat, labels, None, 2)
    assert got["J"][0] == whole["J"][0] and got["F"][0] == whole["F"][0]
    first2 = R.video_validation(flat.reshape(4, T, 2, 7, 9)[1, :2], labels[1:2, :2], None, 2)
    assert got["J"][1] == first2["J"][0] and got["F"][1] == first2["F"][0]
    assert not got["hist"][T + 2:3 * T].any() and not got["stats"][T + 2:3 * T].any()


def test_before_any_update():
    vv = MT.VideoValidation()
    assert vv.counts().shape == (3, 2) and int(vv.counts().sum()) == 0 and vv.videos() == 0
    assert tuple(t.numel() for t in vv.video_scores()) == (0, 0)
    with pytest.raises(CavpError, match="no video"):
        vv.results()
    with pytest.raises(CavpError):
        vv.check()
    vv.reset()


def test_bad_constructor_arguments_raise():
    for kw in (dict(num_classes=1), dict(num_classes=4097), dict(pr_num=0), dict(pr_num=ops.VIDEOVAL_MAX_THRESHOLDS + 1),
               dict(channel=2), dict(channel=-1), dict(max_frames=0), dict(max_frames=65536), dict(max_videos=0)):
        with pytest.raises(CavpError):
            MT.VideoValidation(**kw)
    MT.VideoValidation(num_classes=5, pr_num=ops.VIDEOVAL_MAX_THRESHOLDS, channel=4, ignore_index=None)


def test_cpu_tensors_raise():
    vv = MT.VideoValidation(device="cuda:0")
    lab = torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    with pytest.raises(CavpError, match="CPU"):
        vv.update(torch.zeros(4, 2, 8, 8), lab)
    with pytest.raises(CavpError, match="CPU"):
        vv.update(torch.zeros(4, 2, 8, 8), lab, torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(CavpError, match="CPU"):
        vv.update_lowres(torch.zeros(4, 2, 2, 2), lab)
    with pytest.raises(CavpError):
        MT.VideoValidation(device="cpu").update(torch.zeros(4, 2, 8, 8), lab)
    th = torch.linspace(0, 1, 255)
    stats, hist = torch.zeros(4, 4, dtype=torch.int64), torch.zeros(4, 2, 256, dtype=torch.int32)
    M, state = torch.zeros(6, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(CavpError, match="CPU"):
        ops.videoval_frame_stats(torch.zeros(4, 2, 8, 8), lab, None, 2, 2, 255, th, stats, hist, M, state)
    with pytest.raises(CavpError, match="CPU"):
        ops.videoval_frame_stats(torch.zeros(4, 8, 8, dtype=torch.uint8), lab, None, 2, 2, 255, th, stats, hist, M, state,
                                 prob=torch.zeros(4, 8, 8))
    with pytest.raises(CavpError, match="CPU"):
        ops.videoval_combine(stats, hist, None, 2, 2, 64, 255, torch.zeros(8), torch.zeros(8), state)


def test_malformed_arguments_raise():
    vv = MT.VideoValidation(num_classes=3, max_frames=4, device="cuda:0")
    lab = torch.zeros(2, 2, 8, 8, dtype=torch.int64)
    logits = torch.zeros(4, 3, 8, 8)
    cnt = torch.tensor([1, 2], dtype=torch.int32)
    bad = [
        (logits, lab.int(), None),                                        # labels not int64
        (logits, lab[0, 0], None),                                        # labels 2-d
        (logits, lab.flatten(0, 1), cnt),                                 # count without [B, T, H, W] labels
        (logits[:3], lab, None),                                          # N != B * T
        (logits[:, :, :, :7], lab, None),                                 # H x W differ
        (logits.double(), lab, None),                                     # logits dtype
        (torch.zeros(4, 8, 8, dtype=torch.uint8), lab, None),             # a mask is no input of update()
        (torch.zeros(4, 4, 8, 8), lab, None),                             # num_classes < C
        (torch.zeros(4, 1, 8, 8), lab, None),                             # C < 2
        (torch.zeros(4, 3, 8), lab, None),                                # logits 3-d
        (logits, lab, cnt.float()),                                       # count dtype
        (logits, lab, cnt[:1]),                                           # count shape
        (logits, lab, [1, 2]),                                            # count no tensor
        (torch.zeros(6, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.int64), None),   # N > max_frames
        (logits, lab.transpose(2, 3), None),                              # labels not dense
        (logits.transpose(2, 3), lab, None),                              # logits not dense
    ]
    for pred, labels, count in bad:
        with pytest.raises(CavpError) as e:
            vv.update(pred, labels, count)
        assert "CPU" not in str(e.value), (getattr(pred, "shape", None), labels.shape)   # refused for its own reason
    lo = torch.zeros(4, 2, 2, 3)
    bad_lo = [
        dict(lo=lo[:3], labels=lab),                                      # N != B * T
        dict(lo=lo.double(), labels=lab),                                 # dtype
        dict(lo=lo, labels=lab, input_shape=(8, 9)),                      # input_shape differs from the labels'
        dict(lo=torch.zeros(4, 2, 2, 4), labels=lab),                     # num_classes < C
        dict(lo=lo, labels=lab.flatten(0, 1), count=cnt),                 # count with 3-d labels
    ]
    for kw in bad_lo:
        with pytest.raises(CavpError) as e:
            vv.update_lowres(**kw)
        assert "CPU" not in str(e.value), kw
    with pytest.raises(CavpError, match="channel"):                       # channel 2 of two-channel logits
        MT.VideoValidation(num_classes=3, channel=2, device="cuda:0").update(torch.zeros(4, 2, 8, 8), lab)


def test_ops_argument_checks():
    th = torch.linspace(0, 1, 255)
    lab = torch.zeros(4, 8, 8, dtype=torch.int64)
    stats, hist = torch.zeros(4, 4, dtype=torch.int64), torch.zeros(4, 2, 256, dtype=torch.int32)
    M, state = torch.zeros(6, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    x = torch.zeros(4, 2, 8, 8)
    good = dict(pred=x, labels=lab, count=None, T=2, num_classes=2, ignore=255, thresholds=th, stats=stats, hist=hist, M=M, state=state)
    bad = [
        dict(T=3),                                                        # 4 frames are no whole number of videos of 3
        dict(num_classes=1),                                              # num_classes < C
        dict(channel=2),
        dict(thresholds=torch.linspace(0, 1, ops.VIDEOVAL_MAX_THRESHOLDS + 1)),
        dict(thresholds=th.double()),
        dict(stats=stats[:3]), dict(hist=hist.long()), dict(M=M[:5]), dict(state=state[:4]),
        dict(count=torch.zeros(3, dtype=torch.int32)),
        dict(pred=torch.zeros(4, 8, 8, dtype=torch.uint8)),               # a mask without its probability plane
        dict(prob=torch.zeros(4, 8, 8)),                                  # a plane without a mask
        dict(pred=torch.zeros(4, 8, 8, dtype=torch.uint8), prob=torch.zeros(4, 8, 9)),
        dict(labels=lab[:, :, :7]), dict(labels=lab.int()),
    ]
    for kw in bad:
        with pytest.raises(CavpError) as e:
            ops.videoval_frame_stats(**{**good, **kw})
        assert "CPU" not in str(e.value), kw
    for kw in (dict(J=torch.zeros(8, dtype=torch.float64)), dict(F=torch.zeros(7)), dict(pr_num=0), dict(B=0), dict(stats=stats[:3])):
        args = dict(stats=stats, hist=hist, count=None, B=2, T=2, hw=64, pr_num=255, J=torch.zeros(8), F=torch.zeros(8), state=state)
        with pytest.raises(CavpError) as e:
            ops.videoval_combine(**{**args, **kw})
        assert "CPU" not in str(e.value), kw
