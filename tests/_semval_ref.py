"""numpy restatement of SemanticValidation's specification (cavp_amd/metrics.py, csrc/metrics.hip, include/cavp_hip.h):
the per-frame, per-class IoU / F-score of the reference's utils/avsbench_metrics.py over a batch of clips, on the CPU.  Test
infrastructure only.  Integer counts first, then float32 with one IEEE operation at a time (numpy float32 scalars and arrays: every
operator rounds once), frames in ascending order, classes in ascending order."""
import numpy as np

F32 = np.float32
EPS_UNION = F32(2.220446049250313e-16)
EPS_BINARY = F32(1e-7)


def predictions(pred):
    """Class index per pixel, int64 [N, H, W]: a uint8 class mask as it is, float32 logits [N, C, H, W] by argmax (first maximal
    index, a NaN is the maximum: numpy's argmax)."""
    pred = np.asarray(pred)
    return pred.astype(np.int64) if pred.dtype == np.uint8 else np.argmax(pred, axis=1).astype(np.int64)


def clamp_count(count, B, T):
    return [T] * B if count is None else [min(max(int(c), 0), T) for c in count]


def frame_counts(p, l, K, is_mask=False):
    """(inter [K], pred [K], lab [K], binary [4], bad_mask) of one frame: p, l 1-d int64."""
    P, G = p != 0, l != 0
    binary = np.array([(P & G).sum(), (P | G).sum(), (~P & ~G).sum(), G.sum()], dtype=np.int64)
    ok = p < K if is_mask else np.ones_like(P)
    bad = int((~ok).sum())
    seen = ok & (l >= 0)
    lab_ok = seen & (l < K)
    inter = np.bincount(p[lab_ok & (p == l)], minlength=K)[:K]
    pred = np.bincount(p[seen], minlength=K)[:K]
    lab = np.bincount(l[lab_ok], minlength=K)[:K]
    return inter.astype(np.int64), pred.astype(np.int64), lab.astype(np.int64), binary, bad


def frame_scores(inter, pred, lab):
    """(iou [K], f [K], hit [K], frame_miou) in float32 from one frame's integer areas."""
    with np.errstate(divide="ignore", invalid="ignore"):
        i, p, t = inter.astype(F32), pred.astype(F32), lab.astype(F32)
        union = (p + t) - i
        iou = i / (EPS_UNION + union)
        precision, recall = i / p, i / t
        f = ((F32(1.3) * precision) * recall) / (F32(0.3) * precision + recall)
        f[f != f] = 0
        s = F32(0)
        for v in iou:                       # ascending classes
            s = s + v
        miou = s / F32((iou != 0).sum())    # 0 / 0: the reference's NaN
    assert iou.dtype == F32 and f.dtype == F32 and type(miou) is F32
    return iou, f, union != 0, miou


def binary_iou(binary, hw):
    inter, union = (binary[2], hw) if binary[3] == 0 else (binary[0], binary[1])
    return F32(inter) / (F32(union) + EPS_BINARY)


def call(pred, labels, count, K):
    """One update: pred logits [N, K, H, W] or uint8 mask [N, H, W]; labels int64 [B, T, H, W] or [N, H, W].  Returns a dict of the
    integer scratch `counts` [N, 3K + 4] (zero rows for frames that take no part), the call's float32 partial sums `ious`,
    `fscores`, `cls_count` [K], `frame_miou` [N] (-1: no part), `binary` (the sum of the frames' binary IoU), `frames`, `bad_mask`,
    `bad_count`."""
    pred, labels = np.asarray(pred), np.asarray(labels)
    is_mask = pred.dtype == np.uint8
    B, T = (labels.shape[0], labels.shape[1]) if labels.ndim == 4 else (1, labels.shape[0])
    N, hw = B * T, labels.shape[-1] * labels.shape[-2]
    cl = clamp_count(count, B, T)
    l = labels.reshape(N, -1)
    counts = np.zeros((N, 3 * K + 4), dtype=np.int64)
    ious, fscores, hits = np.zeros(K, F32), np.zeros(K, F32), np.zeros(K, F32)
    frame_miou = np.full(N, -1, F32)
    binary, frames, bad_mask = F32(0), 0, 0
    for n in range(N):
        if n % T >= cl[n // T]:
            continue
        p = predictions(pred[n:n + 1]).reshape(-1)          # only the participating frames are read
        inter, prd, lab, b4, bad = frame_counts(p, l[n], K, is_mask)
        counts[n] = np.concatenate([inter, prd, lab, b4])
        iou, f, hit, frame_miou[n] = frame_scores(inter, prd, lab)
        ious = ious + iou
        fscores = fscores + f
        hits = hits + hit.astype(F32)
        binary = binary + binary_iou(b4, hw)
        frames += 1
        bad_mask += bad
    bad_count = 0 if count is None else sum(int(c) < 0 or int(c) > T for c in count)
    return dict(counts=counts, ious=ious, fscores=fscores, cls_count=hits, frame_miou=frame_miou, binary=F32(binary), frames=frames,
                bad_mask=bad_mask, bad_count=bad_count)


class Accumulator:
    """The running float32 accumulators: each call's partial added as the benchmark driver adds it."""

    def __init__(self, K):
        self.K = K
        self.ious, self.fscores, self.cls_count = np.zeros(K, F32), np.zeros(K, F32), np.zeros(K, F32)
        self.binary, self.frames = F32(0), 0

    def update(self, pred, labels, count=None):
        r = call(pred, labels, count, self.K)
        self.ious = self.ious + r["ious"]
        self.fscores = self.fscores + r["fscores"]
        self.cls_count = self.cls_count + r["cls_count"]
        self.binary = F32(self.binary + r["binary"])
        self.frames += r["frames"]
        return r

    def accumulators(self):
        return np.stack([self.ious, self.fscores, self.cls_count])

    def results(self):
        return results(self.ious, self.fscores, self.cls_count, self.binary, self.frames)


def results(ious, fscores, cls_count, binary, frames):
    """The benchmark driver's reduction in float32."""
    with np.errstate(divide="ignore", invalid="ignore"):
        miou_pc, fscore_pc = ious.astype(F32) / cls_count.astype(F32), fscores.astype(F32) / cls_count.astype(F32)
    miou_pc[miou_pc != miou_pc] = 0
    fscore_pc[fscore_pc != fscore_pc] = 0
    return dict(miou_pc=miou_pc, fscore_pc=fscore_pc, binary_miou=F32(binary) / F32(frames))
