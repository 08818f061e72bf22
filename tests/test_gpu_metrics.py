"""cavp_amd.metrics on the MI355X: the counting kernels (cavp_seg_confusion_nchw, cavp_mask_iou_stats, cavp_fmeasure_hist) against
the reference's own outputs (tests/golden/metrics.npz), a numpy restatement of the confusion counts over a random sweep, and
on-device torch restatements of the reference's mask_iou / Eval_Fmeasure."""
import itertools

import numpy as np
import pytest
import torch

from cavp_amd import metrics as MT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def z(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def _logits(q):
    return torch.from_numpy(q.astype(np.float32) / 8).to(DEV)


# ---- 1. fixture cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["vpo", "avss"])
def test_fixture_seg_metrics_exact(z, case):
    K, C, B, H, W, nb = [int(v) for v in z[f"{case}_meta"]]
    miou, fd = MT.MIoU(num_classes=K, ignore_index=255, local_rank=0), MT.ForegroundDetect(num_classes=K)
    for b in range(nb):
        x, y = _logits(z[f"{case}_logits_q"][b]), torch.from_numpy(z[f"{case}_labels"][b]).to(DEV)
        fd(x, y)
        got = miou(x, y)
        assert tuple(float(v) for v in got) == tuple(z[f"{case}_miou_calls"][b]), (b, got)
    np.testing.assert_array_equal(miou.counts().cpu().numpy(), z[f"{case}_M"])
    np.testing.assert_array_equal(miou.inter.astype(np.float64), z[f"{case}_inter"])
    np.testing.assert_array_equal(miou.union.astype(np.float64), z[f"{case}_union"])
    assert float(miou.correct) == float(z[f"{case}_correct"]) and float(miou.label) == float(z[f"{case}_label"])
    np.testing.assert_array_equal(fd.confusion_matrix_, z[f"{case}_fd_cm"])
    cl = z[f"{case}_class_list"].tolist()
    assert tuple(float(v) for v in fd.get_metric_results()) == tuple(z[f"{case}_fd"])
    assert tuple(float(v) for v in MT.get_performance(miou, fd, cl)) == tuple(z[f"{case}_miou_cl"]) + tuple(z[f"{case}_fd_cl"])


def test_fixture_avs_exact(z):
    x = _logits(z["avs_logits_q"])
    lab = torch.from_numpy(z["avs_labels"]).to(DEV)
    pred = torch.argmax(x, dim=1)
    assert MT.mask_iou(pred, lab).cpu().numpy().tobytes() == z["avs_mask_iou"].tobytes()
    assert MT.mask_iou(pred.float(), lab.float()).cpu().numpy().tobytes() == z["avs_mask_iou_f32"].tobytes()
    prob = torch.from_numpy(z["avs_prob"]).to(DEV)
    hist = torch.zeros((5, 2, 256), dtype=torch.int32, device=DEV)
    from cavp_amd import ops
    ops.fmeasure_hist(prob, lab.float(), MT.thresholds(255, DEV), hist)
    np.testing.assert_array_equal(hist.cpu().numpy(), z["avs_hist"])
    prec, recall, _ = MT.fmeasure_from_hist(hist)
    assert prec.cpu().numpy().tobytes() == z["avs_prec"].tobytes()
    assert recall.cpu().numpy().tobytes() == z["avs_recall"].tobytes()
    assert MT.Eval_Fmeasure(prob, lab.float()) == float(z["avs_fmeasure"])
    assert MT.Eval_Fmeasure(prob, lab) == float(z["avs_fmeasure"])          # int64 gt


# ---- 2. random sweep against a numpy restatement --------------------------------------------------------------------------
def _np_confusion(x, t, K, ignore):
    """First maximal index over C, a NaN counting as the maximum (torch.max); M[(K+1) x K]."""
    x = x.reshape(x.shape[0], x.shape[1], -1)
    nan = np.isnan(x)
    p = np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, x).argmax(1)).ravel()
    t = t.ravel()
    ok = (t >= 0) & (t != ignore)
    row = np.where(t[ok] < K, t[ok], K)
    return np.bincount(row * K + p[ok], minlength=(K + 1) * K).reshape(K + 1, K)


def _sweep_inputs(B, C, K, hw, seed, offset):
    g = np.random.RandomState(seed)
    H, W = hw
    x = (g.randint(-3, 4, size=(B, C, H, W)) / 4).astype(np.float32)        # exact ties
    sel = g.rand(B, C, H, W)
    x[sel < 0.01] = np.inf
    x[(sel >= 0.01) & (sel < 0.02)] = -np.inf
    x[(sel >= 0.02) & (sel < 0.025)] = np.nan
    if H * W > 4:
        x[0, :, 0, :min(W, 3)] = -np.inf                                    # all -inf: index 0
    t = g.randint(0, K, size=(B, H, W)).astype(np.int64)
    ls = g.rand(B, H, W)
    t[ls < 0.05] = 255
    t[(ls >= 0.05) & (ls < 0.1)] = -1
    t[(ls >= 0.1) & (ls < 0.15)] = K + g.randint(0, 3)
    buf = torch.empty(x.size + offset, dtype=torch.float32, device=DEV)
    xt = buf[offset:].view(B, C, H, W)                                      # offset 1: a 4-byte (not 16-byte) aligned view
    xt.copy_(torch.from_numpy(x))
    return x, t, xt, torch.from_numpy(t).to(DEV)


_HW = [(1, 1), (1, 3), (4, 4), (37, 53), (224, 224)]
_SWEEP = [((1, 2, 5)[i % 3], C, kk, hw) for i, (C, kk, hw) in enumerate(itertools.product((2, 22, 71), ("C", "C+2", "150"), _HW))]


@pytest.mark.parametrize("B,C,kk,hw", _SWEEP)
def test_confusion_sweep_exact(B, C, kk, hw):
    K = {"C": C, "C+2": C + 2, "150": 150}[kk]
    for offset in (0, 1):
        x, t, xt, tt = _sweep_inputs(B, C, K, hw, seed=B * 1000 + C * 10 + K + offset, offset=offset)
        m = MT.MIoU(K, 255, 0)
        m.update(xt, tt)
        np.testing.assert_array_equal(m.counts().cpu().numpy(), _np_confusion(x, t, K, 255), err_msg=f"offset {offset}")


@pytest.mark.parametrize("C,K", [(22, 127), (71, 127), (22, 128)])
def test_confusion_largest_lds_histogram_and_first_global(C, K):
    """K = 127 is the largest LDS histogram ((K+1) * K * 4 = 65024 bytes); K = 128 is the first on global atomics."""
    for hw, offset in (((37, 53), 0), ((224, 224), 0), ((37, 53), 1)):
        x, t, xt, tt = _sweep_inputs(2, C, K, hw, seed=C + K + offset, offset=offset)
        m = MT.MIoU(K, 255, 0)
        m.update(xt, tt)
        np.testing.assert_array_equal(m.counts().cpu().numpy(), _np_confusion(x, t, K, 255), err_msg=f"{hw} offset {offset}")


def test_float_labels_count_like_int64():
    """AVS masks arrive as float32 0/1 (ToTensor): counted like the same labels as int64; non-finite labels are not counted."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 4, 37, 52, generator=g).to(DEV)
    yi = torch.randint(0, 6, (3, 37, 52), generator=g)
    yi[:, ::9] = 255
    yf = yi.float()
    yf[0, 1, :5] = float("nan")
    yf[0, 2, :5] = float("inf")
    yi[0, 1, :5] = -1
    yi[0, 2, :5] = -1
    for ws in (slice(None), slice(0, 51)):                   # HW = 37 * 52: 16-byte path; 37 * 51: scalar path
        xs = x[..., ws].contiguous()
        a, b = MT.MIoU(6, 255, 0), MT.MIoU(6, 255, 0)
        a.update(xs, yi[..., ws].contiguous().to(DEV))
        b.update(xs, yf[..., ws].contiguous().to(DEV))
        assert torch.equal(a.counts(), b.counts())


def test_confusion_rejects_fewer_classes_than_channels():
    from cavp_amd._lib import CavpError
    x, y = torch.zeros(1, 5, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(CavpError):
        MT.MIoU(4, 255, 0).update(x, y)


# ---- 3. / 4. target untouched, accumulation ------------------------------------------------------------------------------
def test_target_not_modified_and_accumulation_equals_concatenation():
    g = torch.Generator(device="cpu").manual_seed(3)
    xs = [torch.randn(b, 22, 37, 53, generator=g).to(DEV) for b in (2, 3, 1)]
    ys = [torch.randint(0, 24, (b, 37, 53), generator=g) for b in (2, 3, 1)]
    for y in ys:
        y[:, ::7, ::5] = 255
    ys = [y.to(DEV) for y in ys]
    before = [y.clone() for y in ys]
    many = MT.MIoU(24, 255, 0)
    fdm = MT.ForegroundDetect(24)
    for x, y in zip(xs, ys):
        many(x, y)
        fdm(x, y)
    for y, y0 in zip(ys, before):
        assert torch.equal(y, y0)
    one = MT.MIoU(24, 255, 0)
    res = one(torch.cat(xs), torch.cat(ys))
    assert torch.equal(many.counts(), one.counts())
    assert many.get_metric_results() == res
    fd1 = MT.ForegroundDetect(24)
    fd1(torch.cat(xs), torch.cat(ys))
    np.testing.assert_array_equal(fdm.confusion_matrix_, fd1.confusion_matrix_)
    many.reset()
    assert int(many.counts().sum()) == 0 and many.get_metric_results() == (0.0, 0.0)


# ---- 5. eval forward + update in one graph --------------------------------------------------------------------------------
def test_update_captured_with_eval_forward():
    import types
    from cavp_amd.cavp_model import CAVP
    from cavp_amd.synth import synth_inputs, synth_state_dict
    from cavp_amd.train import _no_gc_during_capture
    C, B, hw = 22, 2, (224, 224)                                              # tests/golden/c1_eval.npz's model
    args = types.SimpleNamespace(seg_model="DeepLabV3Plus", last_three_dilation_stride=[False, True, True], audio_backbone="vgg",
                                 num_classes=C, batch_size=B, local_rank="cpu")
    m = CAVP(50, None, num_classes=C, args=args)
    m.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=1), strict=True)
    m.eval().to(DEV)
    image, audio, _ = synth_inputs(B, hw, num_classes=C, seed=5)
    image, audio = image.to(DEV), audio.to(DEV)
    label = torch.randint(0, 24, (B,) + hw, generator=torch.Generator().manual_seed(9))
    label[:, :8] = 255
    label = label.to(DEV)
    miou, fd = MT.MIoU(24, 255, 0), MT.ForegroundDetect(24)
    with torch.no_grad():
        out, _, _ = m(image, audio, eval_mode=True)
        miou.update(out, label)
        fd.update(out, label)
        torch.cuda.synchronize()
        once_m, once_f = miou.counts().clone(), fd.counts().clone()
        assert int(once_m.sum()) > 0
        miou.reset()
        fd.reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(image, audio, eval_mode=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with _no_gc_during_capture(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
            o, _, _ = m(image, audio, eval_mode=True)
            miou.update(o, label)
            fd.update(o, label)
        miou.reset()
        fd.reset()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(miou.counts(), 3 * once_m)
        assert torch.equal(fd.counts(), 3 * once_f)
        # the results follow the replays: equal to three eager updates of the same batch
        eager_m, eager_f = MT.MIoU(24, 255, 0), MT.ForegroundDetect(24)
        for _ in range(3):
            eager_m.update(out, label)
            eager_f.update(out, label)
        want = eager_m.get_metric_results() + eager_f.get_metric_results()
        assert MT.get_performance(miou, fd) == want
        assert miou.get_metric_results() != (0.0, 0.0)
        # a second "epoch": reset, replay once more
        miou.reset()
        fd.reset()
        assert miou.get_metric_results() == (0.0, 0.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(miou.counts(), once_m)
        one_m, one_f = MT.MIoU(24, 255, 0), MT.ForegroundDetect(24)
        one_m.update(out, label)
        one_f.update(out, label)
        assert MT.get_performance(miou, fd) == one_m.get_metric_results() + one_f.get_metric_results()


# ---- 6. / 7. mask_iou and Eval_Fmeasure against on-device restatements ----------------------------------------------------
def _torch_mask_iou(pred, target, eps=1e-7):
    """The reference's mask_iou (utils/avsbench_utils.py), restated on the device."""
    n, npix = pred.size(0), pred.size(-1) * pred.size(-2)
    empty = target.sum(dim=(1, 2)) == 0
    inter = (pred * target).sum(dim=(1, 2))
    union = torch.maximum(pred, target).sum(dim=(1, 2))
    bg = ((1 - target) * (1 - pred)).sum(dim=(1, 2))
    inter[empty] = bg[empty]
    union[empty] = npix
    return torch.sum(inter / (union + eps)) / n


def _torch_fmeasure(pred, gt, pr_num=255, beta2=0.3):
    """The reference's Eval_Fmeasure / _eval_pr, restated on the device (the threshold table is built on the CPU and moved)."""
    th = torch.linspace(0, 1 - 1e-10, pr_num).to(pred.device)
    total, count, score = 0.0, 0, torch.zeros(pr_num)
    for i in range(pred.size(0)):
        if torch.mean(gt[i]) == 0.0:
            continue
        prec, recall = torch.zeros(pr_num, device=pred.device), torch.zeros(pr_num, device=pred.device)
        for j in range(pr_num):
            above = (pred[i] >= th[j]).float()
            tp = (above * gt[i]).sum()
            prec[j], recall[j] = tp / (above.sum() + 1e-20), tp / (gt[i].sum() + 1e-20)
        f = (1 + beta2) * prec * recall / (beta2 * prec + recall)
        f[f != f] = 0
        total += f
        count += 1
        score = total / count
    return score


def _avs_clip(seed, T=5, hw=(56, 64)):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, 2, *hw, generator=g) * 2
    gt = (torch.rand(T, *hw, generator=g) < 0.3).long()
    gt[1] = 0                                                                # an all-zero gt frame
    return logits.to(DEV), gt.to(DEV)


@pytest.mark.parametrize("seed", [0, 1])
def test_mask_iou_and_fmeasure_bit_equal_to_restatement(seed):
    logits, gt = _avs_clip(seed)
    pred = torch.argmax(logits, dim=1)
    for p, t in ((pred, gt), (pred.float(), gt.float()), (pred, gt.float())):
        assert MT.mask_iou(p, t).cpu().numpy().tobytes() == _torch_mask_iou(p, t).cpu().numpy().tobytes()
    prob = torch.softmax(logits, dim=1)[:, 1].contiguous()
    ref = _torch_fmeasure(prob, gt.float())
    got = MT.fmeasure_curve(prob, gt.float())
    assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()
    assert MT.Eval_Fmeasure(prob, gt.float()) == ref.max().item()
    z = torch.zeros_like(gt)
    assert MT.Eval_Fmeasure(prob, z.float()) == 0.0                         # every frame skipped


def test_fmeasure_logits_input_close_to_softmax_path():
    logits, gt = _avs_clip(4)
    prob = torch.softmax(logits, dim=1)[:, 1].contiguous()
    f_prob = MT.fmeasure_curve(prob, gt.float())
    f_log = MT.fmeasure_curve(logits, gt.float(), channel=1)
    assert float((f_prob - f_log).abs().max()) <= 1e-4
    assert abs(MT.Eval_Fmeasure(logits, gt.float()) - MT.Eval_Fmeasure(prob, gt.float())) <= 1e-4


def test_avs_trainer_expressions():
    """The AVS trainer's literal calls (trainer_cavp_avs_obj.py:317-344): float32 0/1 masks as MIoU / ForegroundDetect targets per
    frame, mask_iou on the argmax, Eval_Fmeasure on the strided view torch.softmax(vid_pred, dim=1)[:, 1, :, :]."""
    logits, gt = _avs_clip(7)                                                # vid_pred [5, 2, H, W]
    pix_label = gt.float().view(1, 5, 1, *gt.shape[1:])                      # [bs, T, 1, H, W] float masks
    miou, fd = MT.MIoU(2, 255, 0), MT.ForegroundDetect(2)
    for i in range(5):
        fd(logits[i:i + 1], pix_label[0, i])
        miou(logits[i:i + 1], pix_label[0, i])
    ref_m, ref_f = MT.MIoU(2, 255, 0), MT.ForegroundDetect(2)
    ref_m.update(logits, gt)
    ref_f.update(logits, gt)
    assert torch.equal(miou.counts(), ref_m.counts()) and torch.equal(fd.counts(), ref_f.counts())
    vid_pred = logits
    miou_i = MT.mask_iou(torch.argmax(vid_pred, dim=1), pix_label[0].squeeze(1))
    assert miou_i.cpu().numpy().tobytes() == _torch_mask_iou(torch.argmax(vid_pred, dim=1), pix_label[0].squeeze(1)).cpu().numpy().tobytes()
    prob = torch.softmax(vid_pred, dim=1)[:, 1, :, :]
    assert not prob.is_contiguous()
    gtf = pix_label.float().squeeze()
    ref = _torch_fmeasure(prob, gtf)
    assert MT.fmeasure_curve(prob, gtf).cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()
    assert MT.Eval_Fmeasure(prob, gtf) == ref.max().item()
