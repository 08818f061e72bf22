"""numpy restatement of VideoValidation's specification (cavp_amd/metrics.py, csrc/metrics.hip, include/cavp_hip.h): the
validation loop of the reference's AVSBench object trainer (trainer_cavp_avs_obj.py:292-363) over a batch of videos, on the CPU.
Test infrastructure only.  The integer part (stats, histograms, confusion counts) is exact; the float32 tail performs the device's
operations one IEEE rounding at a time, in the device's order."""
import numpy as np
import torch

from cavp_amd import metrics as MT

f32 = np.float32
STATE_WORDS = 8


def thresholds(pr_num=255):
    """_eval_pr's table: float32 linspace(0, 1 - 1e-10, pr_num)."""
    return torch.linspace(0, 1 - 1e-10, int(pr_num)).numpy()


def softmax_channel(logits, channel=1):
    """float32 [N, H, W]: the max-subtracted softmax of `channel` of logits [N, C, H, W], the channels summed in ascending order."""
    x = np.asarray(logits, dtype=f32)
    m = x[:, 0]
    for c in range(1, x.shape[1]):
        m = np.fmax(m, x[:, c])
    with np.errstate(invalid="ignore"):
        s = np.zeros_like(m)
        for c in range(x.shape[1]):
            s = s + np.exp(x[:, c] - m)
        return (np.exp(x[:, channel] - m) / s).astype(f32)


def predictions(pred):
    """Class index per pixel, int64 [N, H, W]: a uint8 mask as it is, float32 logits by argmax (first maximum, a NaN is the maximum)."""
    pred = torch.as_tensor(pred)
    return (pred.to(torch.int64) if pred.dtype == torch.uint8 else pred.argmax(1)).numpy()


def confusion(p, t, K, ignore):
    """(K+1) x K counts of the prediction p against the label t (1-d): t >= 0 and t != ignore; row t < K, or K."""
    ok = (t >= 0) & (t != ignore)
    row = np.where(t[ok] < K, t[ok], K)
    return np.bincount(row * K + p[ok], minlength=(K + 1) * K).reshape(K + 1, K).astype(np.int64)


def frame_integers(p, q, t, th, K, ignore, is_mask):
    """One frame (1-d p int64, q float32, t int64) -> (stats int64 [4], hist int64 [2, pr_num + 1], conf int64 [K+1, K], bad labels,
    bad mask bytes)."""
    stats = np.array([(p * t).sum(), np.maximum(p, t).sum(), ((1 - t) * (1 - p)).sum(), t.sum()], dtype=np.int64)
    pr = th.shape[0]
    b = np.searchsorted(th, q, side="right")
    b[np.isnan(q)] = 0
    hist = np.stack([np.bincount(b, minlength=pr + 1), np.bincount(b[t != 0], minlength=pr + 1)]).astype(np.int64)
    keep = p < K if is_mask else np.ones_like(p, dtype=bool)
    bad_label = int(((t != 0) & (t != 1) & (t != ignore)).sum())
    return stats, hist, confusion(p[keep], t[keep], K, ignore), bad_label, int((~keep).sum())


def j_of_video(stats, hw):
    """mask_iou's float32 tail over the frames' stats [c, 4], frames added in ascending order."""
    total = f32(0)
    for o, u, bg, ts in np.asarray(stats).tolist():
        if ts == 0:
            o, u = bg, hw
        total = f32(total + f32(f32(o) / f32(f32(u) + f32(1e-7))))
    return f32(total / f32(len(stats)))


def f_of_video(hists):
    """Eval_Fmeasure's float32 tail over the frames' histograms [c, 2, pr_num + 1]: frames with an all-zero gt are skipped."""
    hists = np.asarray(hists)
    pr = hists.shape[2] - 1
    acc, kept = np.zeros(pr, dtype=f32), 0
    for h in hists:
        suf = h[:, ::-1].cumsum(1)[:, ::-1]
        if suf[1, 0] == 0:
            continue
        kept += 1
        tp = suf[1, 1:].astype(f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            prec = tp / (suf[0, 1:].astype(f32) + f32(1e-20))
            recall = tp / (f32(suf[1, 0]) + f32(1e-20))
            f = ((f32(1.0 + 0.3) * prec) * recall) / (f32(0.3) * prec + recall)
        f[np.isnan(f)] = 0
        acc = (acc + f).astype(f32)
    return f32((acc / f32(kept)).max()) if kept else f32(0)


def means(J, F):
    """The reference's AverageMeter means (unrounded, Python floats): J summed and divided in float32, F in double."""
    total = f32(0)
    for v in np.asarray(J, dtype=f32):
        total = f32(total + v)
    f_sum = 0.0
    for v in np.asarray(F, dtype=f32).tolist():
        f_sum += v
    return float(f32(total / f32(len(J)))), f_sum / len(F)


def video_validation(pred, labels, count, K, ignore=255, pr_num=255, channel=1, prob=None, max_videos=4096, base=0):
    """pred: float32 logits [N, C, H, W], or a uint8 mask [N, H, W] with prob float32 [N, H, W]; labels int64 [B, T, H, W]; count per
    video, or None; base: videos seen before this update.
    -> {"stats" int64 [N, 4], "hist" int64 [N, 2, pr_num+1] (zero for frames that take no part), "M" int64 [K+1, K], "J" / "F"
    float32 lists of the videos stored by this update, "state" the eight state words after it (from zeros, videos seen = base + ...)}."""
    is_mask = torch.as_tensor(pred).dtype == torch.uint8
    lab = np.asarray(labels).astype(np.int64)
    B, T = lab.shape[:2]
    hw = lab.shape[2] * lab.shape[3]
    th = thresholds(pr_num)
    p_all = predictions(pred).reshape(B, T, hw)
    q_all = (np.asarray(prob, dtype=f32) if is_mask else softmax_channel(pred, channel)).reshape(B, T, hw)
    lab = lab.reshape(B, T, hw)
    out = {"stats": np.zeros((B * T, 4), np.int64), "hist": np.zeros((B * T, 2, pr_num + 1), np.int64),
           "M": np.zeros((K + 1, K), np.int64), "J": [], "F": []}
    state = [0] * STATE_WORDS
    state[4] = base
    for b in range(B):
        c = T if count is None else int(count[b])
        if not 0 <= c <= T:
            state[2] += 1
            c = min(max(c, 0), T)
        for i in range(c):
            s, h, m, bl, bm = frame_integers(p_all[b, i], q_all[b, i], lab[b, i], th, K, ignore, is_mask)
            out["stats"][b * T + i], out["hist"][b * T + i] = s, h
            out["M"] += m
            state[0] += bl
            state[1] += bm
        if c == 0:
            continue
        if state[4] < max_videos:
            out["J"].append(j_of_video(out["stats"][b * T:b * T + c], hw))
            out["F"].append(f_of_video(out["hist"][b * T:b * T + c]))
        else:
            state[3] += 1
        state[4] += 1
    out["state"] = state
    return out


def performance(M, class_list=None):
    """get_performance of MIoU / ForegroundDetect reading the counts M, as floats."""
    K = M.shape[1]
    m = torch.from_numpy(np.ascontiguousarray(M))
    return [float(v) for v in MT.get_performance(MT.MIoU(K, 255, 0)._adopt(m), MT.ForegroundDetect(K)._adopt(m), class_list)]
