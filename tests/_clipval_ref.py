"""torch / numpy restatement of ClipValidation's specification (cavp_amd/metrics.py, csrc/metrics.hip): the validation
loop of the reference's AVSS trainers (trainer_cavp_avss_image.py:295-349) over a batch of clips, on the CPU.  Test infrastructure
only.  The keyword switches of `is_multi_source` are deliberate MUTATIONS of the predicate: tests/test_clip_validation_host.py shows
that the fixture tells each of them from the specification."""
import numpy as np
import torch

from cavp_amd import metrics as MT

LABEL_BINS = 256


def predictions(pred):
    """Class index per pixel, int64 [N, H, W]: a uint8 class mask as it is, float32 logits [N, C, H, W] by argmax (first maximum)."""
    pred = torch.as_tensor(pred)
    return (pred.to(torch.int64) if pred.dtype == torch.uint8 else pred.argmax(1)).numpy()


def kept_pixels(p, t, K, is_mask):
    """Pixels that set any bin: the label is < 256 and a mask byte is < K."""
    keep = t < LABEL_BINS
    return keep & (p < K) if is_mask else keep


def confusion(p, t, K, ignore):
    """(K+1) x K counts of the prediction p against the label t (1-d arrays): t >= 0 and t != ignore; row t < K, or K."""
    ok = (t >= 0) & (t != ignore)
    row = np.where(t[ok] < K, t[ok], K)
    return np.bincount(row * K + p[ok], minlength=(K + 1) * K).reshape(K + 1, K).astype(np.int64)


def is_multi_source(t, K, ignore=255, min_count=100, min_values=2, *, at_least=False, skip_ignore=False, lump_large=False):
    """The reference's `uniq_id[count > 100].shape[0] > 2` on one frame's label values t (1-d, already < 256): negative labels are
    the ignore value (the reference's MIoU has overwritten 255 with -1 by the time it calls unique), every other value counts by
    itself.  Mutations: at_least (count >= min_count), skip_ignore (the ignore value is no value), lump_large (values >= K are one)."""
    v = np.where(t < 0, ignore, t)
    if skip_ignore:
        v = v[v != ignore]
    if lump_large:
        v = np.where((v >= K) & (v != ignore), K, v)
    _, cnt = np.unique(v, return_counts=True)
    return int((cnt >= min_count if at_least else cnt > min_count).sum()) > min_values


def clip_validation(pred, labels, count, K, ignore=255, min_count=100, min_values=2, **mutation):
    """pred: uint8 mask [N, H, W] or float32 logits [N, C, H, W]; labels int64 [B, T, H, W]; count: per clip, or None.
    -> {"counts" int64 [2, K+1, K] (ALL, MS), "frames" (ALL, MS), "bad" [labels >= 256, mask bytes >= K, counts outside [0, T]]}."""
    is_mask = torch.as_tensor(pred).dtype == torch.uint8
    lab = np.asarray(labels).astype(np.int64)
    B, T = lab.shape[:2]
    p_all = predictions(pred).reshape(B, T, -1)
    lab = lab.reshape(B, T, -1)
    counts = np.zeros((2, K + 1, K), dtype=np.int64)
    frames, bad = [0, 0], [0, 0, 0]
    for b in range(B):
        c = T if count is None else int(count[b])
        if not 0 <= c <= T:
            bad[2] += 1
            c = min(max(c, 0), T)
        for i in range(c):
            p, t = p_all[b, i], lab[b, i]
            bad[0] += int((t >= LABEL_BINS).sum())
            if is_mask:
                bad[1] += int(((t < LABEL_BINS) & (p >= K)).sum())
            keep = kept_pixels(p, t, K, is_mask)
            p, t = p[keep], t[keep]
            m = confusion(p, t, K, ignore)
            counts[0] += m
            frames[0] += 1
            if is_multi_source(t, K, ignore, min_count, min_values, **mutation):
                counts[1] += m
                frames[1] += 1
    return {"counts": counts, "frames": tuple(frames), "bad": bad}


def results(counts, class_list=None):
    """The ten rounded results of a [2, K+1, K] count pair as floats: get_performance of MIoU / ForegroundDetect reading them."""
    K = counts.shape[2]
    out = []
    for m in counts:
        M = torch.from_numpy(np.ascontiguousarray(m))
        perf = MT.get_performance(MT.MIoU(K, 255, 0)._adopt(M), MT.ForegroundDetect(K)._adopt(M), class_list)
        out += [float(v) for v in perf]
    return out
