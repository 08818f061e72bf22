"""CPU checks of cavp_amd.metrics: the host finalisation reproduces every reference value stored in tests/golden/metrics.npz
(tools/make_golden_metrics.py ran the reference's utils/eval_utils.py and utils/avsbench_utils.py) from the integer counts the
kernels produce, and the API refuses CPU tensors and malformed shapes."""
import os

import numpy as np
import pytest
import torch

from cavp_amd._lib import CavpError
from cavp_amd import metrics as MT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _with_counts(obj, M):
    obj._M = torch.from_numpy(np.ascontiguousarray(M).ravel().copy())   # host copy of what the kernel accumulates
    return obj


@pytest.mark.parametrize("case", ["vpo", "avss"])
def test_miou_finalisation_matches_reference(z, case):
    K = int(z[f"{case}_meta"][0])
    m = _with_counts(MT.MIoU(num_classes=K, ignore_index=255, local_rank=0), z[f"{case}_M"])
    miou, acc = m.get_metric_results()
    assert (float(miou), float(acc)) == tuple(z[f"{case}_miou_calls"][-1])
    np.testing.assert_array_equal(m.inter.astype(np.float64), z[f"{case}_inter"])
    np.testing.assert_array_equal(m.union.astype(np.float64), z[f"{case}_union"])
    assert float(m.correct) == float(z[f"{case}_correct"]) and float(m.label) == float(z[f"{case}_label"])
    cl = z[f"{case}_class_list"].tolist()
    assert tuple(float(v) for v in m.get_metric_results(cl)) == tuple(z[f"{case}_miou_cl"])


@pytest.mark.parametrize("case", ["vpo", "avss"])
def test_foreground_detect_finalisation_matches_reference(z, case):
    K = int(z[f"{case}_meta"][0])
    fd = _with_counts(MT.ForegroundDetect(num_classes=K), z[f"{case}_M"])
    np.testing.assert_array_equal(fd.confusion_matrix_, z[f"{case}_fd_cm"])
    assert tuple(float(v) for v in fd.get_metric_results()) == tuple(z[f"{case}_fd"])
    cl = z[f"{case}_class_list"].tolist()
    assert tuple(float(v) for v in fd.get_metric_results(cl)) == tuple(z[f"{case}_fd_cl"])
    m = _with_counts(MT.MIoU(K, 255, 0), z[f"{case}_M"])
    perf = MT.get_performance(m, fd, cl)
    assert tuple(float(v) for v in perf) == tuple(z[f"{case}_miou_cl"]) + tuple(z[f"{case}_fd_cl"])


def test_before_any_update_matches_reference_constructor_state():
    m = MT.MIoU(24, 255, 0)
    assert m.get_metric_results() == (0.0, 0.0)
    assert m.counts().shape == (25, 24) and int(m.counts().sum()) == 0


def _mask_stats(p, t):
    p, t = p.reshape(p.shape[0], -1).astype(np.int64), t.reshape(t.shape[0], -1).astype(np.int64)
    return torch.from_numpy(np.stack([(p * t).sum(1), np.maximum(p, t).sum(1), ((1 - t) * (1 - p)).sum(1), t.sum(1)], 1))


def test_mask_iou_finalisation_matches_reference(z):
    pred = torch.from_numpy(z["avs_logits_q"].astype(np.float32)).argmax(1).numpy()
    lab = z["avs_labels"]
    stats = _mask_stats(pred, lab)
    hw = lab.shape[1] * lab.shape[2]
    got = MT.mask_iou_from_stats(stats, hw, torch.int64)
    assert got.dtype == torch.float32 and got.numpy().tobytes() == z["avs_mask_iou"].tobytes()
    got = MT.mask_iou_from_stats(stats, hw, torch.float32)
    assert got.numpy().tobytes() == z["avs_mask_iou_f32"].tobytes()


def test_fmeasure_finalisation_matches_reference(z):
    prec, recall, score = MT.fmeasure_from_hist(torch.from_numpy(z["avs_hist"]))
    assert prec.numpy().tobytes() == z["avs_prec"].tobytes()
    assert recall.numpy().tobytes() == z["avs_recall"].tobytes()
    assert score.max().item() == float(z["avs_fmeasure"])


def test_fmeasure_all_frames_empty_is_zero():
    h = torch.zeros((3, 2, 256), dtype=torch.int64)
    h[:, 0, 7] = 100            # pixels, but no foreground anywhere: every frame is skipped
    assert MT.fmeasure_from_hist(h)[2].max().item() == 0.0


def test_cpu_tensors_raise():
    x, y = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(CavpError):
        MT.MIoU(3, 255, 0)(x, y)
    with pytest.raises(CavpError):
        MT.ForegroundDetect(3)(x, y)
    with pytest.raises(CavpError):
        MT.mask_iou(y, y)
    with pytest.raises(CavpError):
        MT.Eval_Fmeasure(torch.zeros(2, 8, 8), y.float())


def test_bad_shapes_raise():
    x = torch.zeros(2, 3, 8, 8)
    for y in (torch.zeros(2, 1, 8, 8, dtype=torch.int64), torch.zeros(3, 8, 8, dtype=torch.int64),
              torch.zeros(2, 8, 9, dtype=torch.int64)):
        with pytest.raises(CavpError, match="target"):
            MT.MIoU(3, 255, 0)(x, y)
    with pytest.raises(CavpError, match="one shape"):
        MT.mask_iou(torch.zeros(2, 8, 8), torch.zeros(2, 8, 9))
    with pytest.raises(CavpError, match="gt"):
        MT.Eval_Fmeasure(torch.zeros(2, 8, 8), torch.zeros(3, 8, 8))
