"""Validation metrics on the GPU, under the reference's names (utils/eval_utils.py: MIoU, ForegroundDetect, get_performance;
utils/avsbench_utils.py: mask_iou, Eval_Fmeasure).

The counting runs in libcavp_hip.so (cavp_seg_confusion_nchw, cavp_mask_iou_stats, cavp_fmeasure_hist): one pass over the
logits / masks, exact integer counts.  What the reference computes in floating point from those counts (IoU, accuracy, FDR,
F-beta, the precision / recall curves) is done here in the reference's dtypes and operation order, so the results equal the
reference's as long as its own float32 accumulators are exact: MIoU's per-class sums stay below 2^24 pixels (a few hundred
224^2 frames for the largest class).  Beyond that the reference's float32 sums round; the int64 counts here do not.

    from cavp_amd.metrics import MIoU, ForegroundDetect, get_performance, mask_iou, Eval_Fmeasure

Differences from the reference, on purpose:
  * the target is never written to (MIoU.__call__ of the reference stores -1 into the caller's ignore pixels);
  * targets must be [B, H, W] with B, H, W of the logits [B, C, H, W], int64 or float32 holding integers (AVS masks);
    anything else raises CavpError;
  * MIoU.inter / .union / .correct / .label are exact int64 counts (float32 arrays in the reference);
  * Eval_Fmeasure treats gt as a binary mask (gt != 0), as the AVS trainers feed it;
  * mask_iou's float inputs must be masks (integer values): each pixel is truncated to an integer before summing;
  * device tensors only: there is no CPU path (CavpError).
Additions: `update_lowres(lo, y)` (the same counts from the model's low-resolution logits, CAVP.predict_lowres: the full-resolution
logits are never written), `update(x, y)` (no host sync; no allocation after the first call, so it can be captured in a hipGraph with the eval
forward), `reset()`, `counts()` (the device-side (K+1) x K confusion counts) and `fmeasure_curve(...)` (the score curve as a
device tensor, without `.item()`), and `ClipValidation`: the validation loop of the AVSS trainers (trainer_cavp_avss_image.py:295-349)
for whole batches of clips - every frame counted into an ALL matrix and, when its own label histogram says "multi-source", into an
MS matrix as well, decided on the device; and `VideoValidation`: the validation loop of the AVSBench object trainer
(trainer_cavp_avs_obj.py:292-363) - per-video J (mask_iou) and F (Eval_Fmeasure) of whole batches of videos, finished on the device;
and `SemanticValidation`: the AVSBench-semantic metric (utils/avsbench_metrics.py) - per-frame, per-class IoU and F-score of whole
batches of clips, with `calc_color_miou_fscore` / `calc_color_miou` / `calc_binary_miou` under the reference's names."""
from __future__ import annotations

import numpy
import torch

from . import ops
from ._lib import CavpError
from .train_ops import zero_ as _zero_
from .train_ops import zeros as _zeros

__all__ = ["MIoU", "ForegroundDetect", "get_performance", "mask_iou", "Eval_Fmeasure", "fmeasure_curve", "ClipValidation",
           "VideoValidation", "SemanticValidation", "calc_color_miou_fscore", "calc_color_miou", "calc_binary_miou"]


def get_performance(miou_measure_in, fg_measure_in, class_list=None):
    """(mIoU, acc, FDR, F1, F0.3) of the two accumulators."""
    return (*miou_measure_in.get_metric_results(class_list), *fg_measure_in.get_metric_results(class_list))


def iou_and_accuracy(M: numpy.ndarray):
    """Per-class IoU (float64 [K]) and pixel accuracy (float64) from the (K+1) x K counts M: intersection = diagonal, union =
    predicted + labelled - intersection (row K holds valid labels >= K, predicted but never labelled as a class), accuracy =
    trace / all counted pixels, each over (spacing(1) + denominator) in float64."""
    k = M.shape[1]
    hits = numpy.diag(M[:k]).astype(numpy.int64)
    union = M.sum(0) + M[:k].sum(1) - hits
    eps = numpy.spacing(1)
    return hits, union, hits.astype(numpy.float64) / (union + eps), float(numpy.trace(M[:k])) / (M.sum() + eps)


def pixel_scores(iou: numpy.ndarray, acc, class_list=None):
    """(mIoU, acc) rounded to 4 decimals from the per-class IoU and the accuracy; mIoU over `class_list` when given."""
    iou = iou if class_list is None else iou[class_list]
    return numpy.round(iou.mean().item(), 4), numpy.round(acc, 4)


def detection_scores(cm: torch.Tensor, class_list=None):
    """(FDR, F1, F0.3) of a float64 K x K confusion matrix (rows: label, columns: prediction), nan-means over the classes
    (or over `class_list`), each rounded to 4 decimals as a 0-d numpy array."""
    hits = torch.diag(cm)
    false_pos = cm.sum(dim=0) - hits
    missed = cm.sum(dim=1) - hits
    if class_list is not None:
        hits, false_pos, missed = hits[class_list], false_pos[class_list], missed[class_list]

    def f_beta(b2):
        weighted = (1 + b2) * hits
        return torch.nanmean(weighted / (weighted + b2 * missed + false_pos))

    scores = (torch.nanmean(false_pos / (false_pos + hits)), f_beta(1.0), f_beta(0.3))
    return tuple(torch.round(v, decimals=4).cpu().numpy() for v in scores)


class _Confusion:
    """(K+1) x K int64 counts on the device: M[t][p] for labels t < K, M[K][p] for valid labels >= K (cavp_seg_confusion_nchw)."""

    def _init_counts(self, num_classes: int, ignore):
        self.num_classes = int(num_classes)
        self._kernel_ignore = -1 if ignore is None else int(ignore)   # -1 is never a valid label (t >= 0)
        self._M = None

    def _counts_on(self, device) -> torch.Tensor:
        """The counts the kernels add into: zeros on `device` at the first update (and after a change of device)."""
        if self._M is None or self._M.device != device:
            k = self.num_classes
            self._M = _zeros(((k + 1) * k,), torch.int64, device)
        return self._M

    def update(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """Accumulate one batch: x logits [B, C, H, W] (float32), y labels [B, H, W] (int64, or float32 holding integers).
        No host sync; graph replays of a captured update() accumulate the same way."""
        if x.dim() != 4 or y.dim() != 3 or y.shape[0] != x.shape[0] or tuple(y.shape[1:]) != tuple(x.shape[2:]):
            raise CavpError(f"{type(self).__name__}: logits [B, C, H, W] and target [B, H, W] required, got "
                            f"{tuple(x.shape)} / {tuple(y.shape)}")
        ops._need_gpu(x, y)
        ops.seg_confusion(x.detach(), y, self.num_classes, self._kernel_ignore, self._counts_on(x.device))

    def update_lowres(self, lo: torch.Tensor, y: torch.Tensor, input_shape=None, align_corners: bool = False) -> None:
        """update() from the low-resolution logits `lo` (NHWC view [B, h, w, C], f32 or bf16: CAVP.predict_lowres): the counts of
        update(full_res_logits, y) where full_res_logits is the bilinear upsample of `lo` to `input_shape` (default y.shape[1:]),
        which is never materialised (ops.seg_predict).  No host sync, no allocation after the first call."""
        if lo.dim() != 4 or y.dim() != 3 or y.shape[0] != lo.shape[0]:
            raise CavpError(f"{type(self).__name__}: low-res logits [B, h, w, C] and target [B, H, W] required, got "
                            f"{tuple(lo.shape)} / {tuple(y.shape)}")
        shape = tuple(y.shape[1:]) if input_shape is None else tuple(int(v) for v in input_shape)
        if shape != tuple(y.shape[1:]):
            raise CavpError(f"{type(self).__name__}: input_shape {shape} differs from the target's {tuple(y.shape[1:])}")
        ops._need_gpu(lo, y)
        ops.seg_predict(lo.detach(), shape, labels=y, num_classes=self.num_classes, ignore=self._kernel_ignore,
                        M=self._counts_on(lo.device), align_corners=align_corners)

    def counts(self) -> torch.Tensor:
        """The (K+1) x K confusion counts (int64, on the device; zeros on the CPU before the first update)."""
        k = self.num_classes
        if self._M is None:
            return torch.zeros((k + 1, k), dtype=torch.int64)
        return self._M.view(k + 1, k)

    def reset(self) -> None:
        if self._M is not None:
            _zero_(self._M)

    def _host_counts(self) -> numpy.ndarray:
        return self.counts().cpu().numpy()

    def _adopt(self, M: torch.Tensor):
        """Read the (K+1) * K int64 counts `M` that someone else owns and updates (ClipValidation) instead of counts of its own:
        no copy, every read of this object sees M's current values."""
        ops._check_counts(M, self.num_classes, "_adopt")
        self._M = M.view(-1)
        return self


class MIoU(_Confusion):
    """Mean IoU and pixel accuracy over all batches seen (labels == ignore_index and negative labels are not counted)."""

    def __init__(self, num_classes, ignore_index, local_rank):
        self.ignore_index = ignore_index
        self.local_rank = local_rank
        self._init_counts(num_classes, ignore_index)
        self._refresh()

    def _refresh(self):
        """inter / union / correct / label, iou and acc from the current device counts (one host copy); the constructor's zeros
        before the first update.  Always read afresh: graph replays and reset() change the counts behind Python's back."""
        if self._M is None:
            self.inter, self.union, self.correct, self.label = 0, 0, 0, 0
            self.iou, self.acc = numpy.zeros(self.num_classes, dtype=numpy.int64), 0.0
            return
        M = self._host_counts()
        self.inter, self.union, self.iou, self.acc = iou_and_accuracy(M)
        self.correct, self.label = int(numpy.trace(M[: self.num_classes])), int(M.sum())

    def get_metric_results(self, class_list=None):
        """(mIoU, acc) rounded to 4 decimals; mIoU over `class_list` when given."""
        self._refresh()
        return pixel_scores(self.iou, self.acc, class_list)

    def __call__(self, x, y):
        self.update(x, y)
        return self.get_metric_results()


class ForegroundDetect(_Confusion):
    """Per-class false discovery rate and F-scores from the label x prediction confusion matrix over all batches seen."""

    def __init__(self, num_classes, ignore_class=255, local_rank=0):
        self.ignore = ignore_class
        self.local_rank = local_rank
        self._init_counts(num_classes, ignore_class)

    @property
    def confusion_matrix_(self) -> numpy.ndarray:
        """The reference's float64 K x K matrix (rows: label, columns: prediction); a host copy of the device counts."""
        return self._host_counts()[: self.num_classes].astype(numpy.float64)

    def get_metric_results(self, class_list=None):
        """(FDR, F1, F0.3) rounded to 4 decimals (0-d numpy arrays); over `class_list` when given."""
        return detection_scores(torch.tensor(self.confusion_matrix_), class_list)

    def __call__(self, y_hat, y):
        self.update(y_hat, y)


def mask_iou_from_stats(stats: torch.Tensor, num_pixels: int, dtype: torch.dtype, eps: float = 1e-7) -> torch.Tensor:
    """mask_iou's tail from the per-image sums stats[N, 4] = (sum p*t, sum max(p, t), sum (1-t)(1-p), sum t) in `dtype`, the dtype
    of the reference's sums (torch.result_type(pred, target)): a frame with an empty target scores its background overlap over
    all pixels; the mean over frames of overlap / (union + eps)."""
    if dtype != torch.int64:
        stats = stats.to(dtype)
    overlap, union, bg_overlap, t_sum = stats.unbind(1)
    empty = t_sum == 0
    overlap = torch.where(empty, bg_overlap, overlap)
    union = union.masked_fill(empty, num_pixels)
    return torch.sum(overlap / (union + eps)) / stats.shape[0]


def mask_iou(pred, target, eps=1e-7, size_average=True):
    """Mean IoU of binary masks pred / target [N, H, W] (int64 or float32) as a 0-d device tensor; size_average is accepted and
    unused.  Float inputs must hold integers: each pixel is truncated to an integer before summing, so a probability map gives a
    different answer from the reference, which sums the floats."""
    if len(pred.shape) != 3 or pred.shape != target.shape:
        raise CavpError(f"mask_iou: pred and target must be [N, H, W] of one shape, got {tuple(pred.shape)} / {tuple(target.shape)}")
    ops._need_gpu(pred, target)
    n = pred.size(0)
    stats = ops.mask_iou_stats(pred, target, _zeros((n, 4), torch.int64, pred.device))
    return mask_iou_from_stats(stats, pred.size(-1) * pred.size(-2), torch.result_type(pred, target), eps)


_thresholds = {}


def thresholds(pr_num: int, device) -> torch.Tensor:
    """_eval_pr's threshold table: torch.linspace(0, 1 - 1e-10, pr_num) built on the CPU and moved to the device, as the reference
    does (cached; the histogram kernel needs it ascending, checked once)."""
    key = (torch.device(device), int(pr_num))
    th = _thresholds.get(key)
    if th is None:
        if key[0].type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise CavpError("fmeasure thresholds would be built during hipGraph capture; run one eager call first")
        host = torch.linspace(0, 1 - 1e-10, int(pr_num))
        if pr_num > 1 and not bool((host[1:] >= host[:-1]).all()):
            raise CavpError("fmeasure: threshold table is not ascending")
        th = host.to(device)
        _thresholds[key] = th
    return th


def fmeasure_from_hist(hist: torch.Tensor, beta2: float = 0.3):
    """Eval_Fmeasure's arithmetic from the per-image histograms hist[N, 2, pr_num + 1] (cavp_fmeasure_hist), on hist's device.
    Returns (prec [N, pr_num], recall [N, pr_num], score [pr_num]); frames whose gt is all zero are skipped as in the reference.
    Suffix sums of the histogram are y_temp.sum() and tp of every threshold; the float32 steps are the reference's."""
    h = hist.to(torch.int64)
    suf = h.flip(-1).cumsum(-1).flip(-1)           # suf[..., b] = #pixels with bin >= b
    n = h.shape[0]
    tp = suf[:, 1, 1:].float()                     # (y_temp * y).sum() for threshold i: bin >= i + 1
    prec = tp / (suf[:, 0, 1:].float() + 1e-20)
    ysum = suf[:, 1, :1].float()
    recall = tp / (ysum + 1e-20)
    f_score = (1 + beta2) * prec * recall / (beta2 * prec + recall)
    f_score = f_score.masked_fill(f_score != f_score, 0)
    valid = ysum[:, 0] > 0
    avg_f = torch.where(valid[0], f_score[0], 0.0)
    for i in range(1, n):
        avg_f = avg_f + torch.where(valid[i], f_score[i], 0.0)
    img_num = valid.sum().float()
    # `avg_f / img_num` with a Python int: torch multiplies a device tensor by the float32 reciprocal, a CPU tensor it divides
    score = avg_f * (1.0 / img_num) if avg_f.is_cuda else avg_f / img_num
    score = torch.where(img_num > 0, score, 0.0)
    return prec, recall, score


def fmeasure_curve(pred, gt, pr_num=255, channel=1, hist_out=None) -> torch.Tensor:
    """Eval_Fmeasure's averaged score curve [pr_num] as a device tensor (no host sync).  pred: probabilities [N, H, W] with dense
    H x W planes (the images may be strided, e.g. torch.softmax(logits, 1)[:, 1]), or logits [N, C, H, W] whose softmax channel `channel` is the probability (computed in the kernel).  gt: [N, H, W] float32 or
    int64 binary mask.  hist_out: optional int32 [N, 2, pr_num + 1] buffer (cleared here) for graph capture."""
    if pred.dim() not in (3, 4) or gt.dim() != 3 or gt.shape[0] != pred.shape[0] or tuple(gt.shape[1:]) != tuple(pred.shape[-2:]):
        raise CavpError(f"Eval_Fmeasure: pred [N, H, W] (or logits [N, C, H, W]) and gt [N, H, W] required, got "
                        f"{tuple(pred.shape)} / {tuple(gt.shape)}")
    ops._need_gpu(pred, gt)
    th = thresholds(pr_num, pred.device)
    shape = (pred.shape[0], 2, int(pr_num) + 1)
    hist = _zeros(shape, torch.int32, pred.device) if hist_out is None else _zero_(hist_out)
    ops.fmeasure_hist(pred, gt, th, hist, channel)
    return fmeasure_from_hist(hist)[2]


def Eval_Fmeasure(pred, gt, measure_path="", pr_num=255, channel=1):
    """Best F-measure (beta^2 = 0.3) over `pr_num` thresholds, averaged over the frames whose gt is not all zero, as a Python
    float.  pred: probabilities [N, H, W] (dense H x W planes; a strided view such as torch.softmax(logits, 1)[:, 1] is read in
    place) or logits [N, C, H, W] (softmax channel `channel` taken in the kernel); gt: binary mask [N, H, W].  measure_path is
    accepted and unused."""
    return fmeasure_curve(pred, gt, pr_num, channel).max().item()


MAX_CLASSES = 4096                 # CAVP_METRICS_MAX_CLASSES
MAX_CLIP_FRAMES = 65535            # frames of one update(): the launch grid's second dimension
MAX_CLIP_SCRATCH = 4 << 30         # bytes of per-frame scratch one ClipValidation may ask for


class ClipValidation:
    """The validation loop of the AVSS trainers (trainer_cavp_avss_image.py:295-349) for whole batches of clips, without the host:

        cv = ClipValidation(num_classes=K, ignore_index=255, min_count=100, min_values=2, max_frames=320, device="cuda:0")
        cv.update(model.predict(image, audio), labels, count)
        (miou, acc, fdr, f1, f03), (miou_ms, acc_ms, fdr_ms, f1_ms, f03_ms) = cv.results()

    labels: dense int64 [B, T, H, W] (or [N, H, W] with count=None); never written.  pred: the dense uint8 class mask [B*T, H, W]
    of CAVP.predict, or dense float32 logits [B*T, C, H, W] (argmax: first maximal index, a NaN is the maximum).  count: device
    int32 / int64 [B], the reference's mask_num per clip: frame t of clip b takes part iff t < count[b] (None: every frame); a
    frame that takes no part is not read.

    Every participating frame adds its confusion counts (the (K+1) x K bin rule of MIoU / ForegroundDetect) to the ALL matrix.  It
    is multi-source, and adds them to the MS matrix too, iff more than `min_values` distinct label values have more than
    `min_count` pixels in it - the reference's `uniq_id[count > 100].shape[0] > 2` on the frame's raw label: the ignore value is a
    value (negative labels fall into its bin: the reference's MIoU has turned 255 into -1 by then), values >= K are values of their
    own, the domain is [0, 256).  A pixel whose label is >= 256 or whose mask byte is >= K sets no bin at all, a count[b] outside
    [0, T] is clamped; each is counted on the device, and check() raises if there were any.

    update() does no host sync and allocates nothing after the first call: it can be captured in a hipGraph with CAVP.predict
    (run one eager update first).  Three launches (csrc/metrics.hip); integer adds only, so the counts do not depend
    on arrival order.  all_miou / all_fg / ms_miou / ms_fg are MIoU / ForegroundDetect objects that read the device counts of this
    object (no copies)."""

    def __init__(self, num_classes: int, ignore_index: int = 255, min_count: int = 100, min_values: int = 2, max_frames: int = 320,
                 device=None):
        k = int(num_classes)
        if not 1 <= k <= MAX_CLASSES:
            raise CavpError(f"ClipValidation: 1 <= num_classes <= {MAX_CLASSES}, got {num_classes}")
        if ignore_index is None or not 0 <= int(ignore_index) < 256:
            raise CavpError(f"ClipValidation: 0 <= ignore_index < 256, got {ignore_index}")
        if int(min_count) < 0 or int(min_values) < 0 or int(min_count) >= 2 ** 31 or int(min_values) >= 2 ** 31:
            raise CavpError("ClipValidation: min_count and min_values are non-negative int32 values")
        if not 1 <= int(max_frames) <= MAX_CLIP_FRAMES:
            raise CavpError(f"ClipValidation: 1 <= max_frames <= {MAX_CLIP_FRAMES}")
        self.num_classes, self.ignore_index = k, int(ignore_index)
        self.min_count, self.min_values, self.max_frames = int(min_count), int(min_values), int(max_frames)
        self.nbins = (k + 1) * k
        self.scratch_bytes = self.max_frames * (self.nbins + 256) * 4
        if self.scratch_bytes > MAX_CLIP_SCRATCH:
            raise CavpError(f"ClipValidation: {self.scratch_bytes} bytes of per-frame scratch for num_classes={k}, "
                            f"max_frames={max_frames}; lower max_frames")
        self._device = device
        self._counts = None          # device buffers, allocated by the first update (the constructor touches no device)
        self.all_miou, self.ms_miou = (MIoU(k, self.ignore_index, 0) for _ in range(2))
        self.all_fg, self.ms_fg = (ForegroundDetect(k, self.ignore_index, 0) for _ in range(2))

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _bind(self, hist, conf, flags, counts, frames, state):
        """Take the device buffers: hist u32 [max_frames, 256] and conf u32 [max_frames, (K+1)K] (as int32; zero at rest), flags
        [max_frames] int32, counts int64 [2, K+1, K], frames int64 [2], state int64 [4]; the four accessors read `counts`."""
        k, mf = self.num_classes, self.max_frames
        want = ((hist, torch.int32, mf * 256), (conf, torch.int32, mf * self.nbins), (flags, torch.int32, mf),
                (counts, torch.int64, 2 * self.nbins), (frames, torch.int64, 2), (state, torch.int64, 4))
        for t, dt, numel in want:
            if t.dtype != dt or t.numel() != numel or not t.is_contiguous() or not t.is_cuda or t.device != hist.device:
                raise CavpError("ClipValidation: device buffers of the wrong dtype, size or device")
        self.device = hist.device
        self._hist, self._conf, self._flags, self._frames, self._state = hist, conf, flags, frames, state
        self._counts = counts.view(2, k + 1, k)
        self.all_miou._adopt(self._counts[0])
        self.all_fg._adopt(self._counts[0])
        self.ms_miou._adopt(self._counts[1])
        self.ms_fg._adopt(self._counts[1])

    def _ensure(self):
        if self._counts is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise CavpError("ClipValidation lives on a HIP device (there is no CPU fallback)")
            if torch.cuda.is_current_stream_capturing():
                raise CavpError("ClipValidation would allocate during hipGraph capture; run one eager update first")
            mf = self.max_frames
            self._bind(_zeros((mf, 256), torch.int32, dev), _zeros((mf, self.nbins), torch.int32, dev),
                       _zeros((mf,), torch.int32, dev), _zeros((2 * self.nbins,), torch.int64, dev),
                       _zeros((2,), torch.int64, dev), _zeros((4,), torch.int64, dev))

    # ---- the update --------------------------------------------------------------------------------------------------------
    def _check_inputs(self, pred, labels, count):
        E = CavpError
        if not isinstance(pred, torch.Tensor) or not isinstance(labels, torch.Tensor):
            raise E("ClipValidation: pred and labels are tensors")
        if labels.dtype != torch.int64 or labels.dim() not in (3, 4):
            raise E(f"ClipValidation: labels must be int64 [B, T, H, W] (or [N, H, W] without count), got {labels.dtype} "
                    f"{tuple(labels.shape)}")
        if labels.dim() == 3 and count is not None:
            raise E("ClipValidation: count needs labels [B, T, H, W]")
        B, T = (labels.shape[0], labels.shape[1]) if labels.dim() == 4 else (1, labels.shape[0])
        H, W = labels.shape[-2:]
        N = B * T
        if N < 1 or H < 1 or W < 1:
            raise E("ClipValidation: empty labels are not supported")
        if N > self.max_frames:
            raise E(f"ClipValidation: {N} frames in one update, max_frames = {self.max_frames}")
        is_mask = pred.dtype == torch.uint8
        if is_mask:
            if tuple(pred.shape) != (N, H, W):
                raise E(f"ClipValidation: a uint8 class mask of shape {(N, H, W)} required, got {tuple(pred.shape)}")
            c = 0
        elif pred.dtype == torch.float32:
            if pred.dim() != 4 or pred.shape[0] != N or tuple(pred.shape[2:]) != (H, W):
                raise E(f"ClipValidation: float32 logits [{N}, C, {H}, {W}] required, got {tuple(pred.shape)}")
            c = pred.shape[1]
            if not 1 <= c <= self.num_classes:
                raise E(f"ClipValidation: num_classes {self.num_classes} < logit channels {c}")
        else:
            raise E(f"ClipValidation: pred is a uint8 class mask [N, H, W] or float32 logits [N, C, H, W], got {pred.dtype}")
        if count is not None:
            if not isinstance(count, torch.Tensor) or count.dtype not in (torch.int32, torch.int64) or tuple(count.shape) != (B,):
                raise E(f"ClipValidation: count must be an int32 or int64 tensor of shape ({B},)")
        if not (pred.is_contiguous() and labels.is_contiguous() and (count is None or count.is_contiguous())):
            raise E("ClipValidation: dense (contiguous) tensors required")
        ops._need_gpu(pred, labels, count)
        return B, T, c, H * W, is_mask

    def update(self, pred: torch.Tensor, labels: torch.Tensor, count=None) -> None:
        """Count one batch of clips (see the class docstring).  No host sync; graph replays of a captured update() accumulate the
        same way."""
        B, T, c, HW, is_mask = self._check_inputs(pred, labels, count)
        self._ensure()
        for t in (pred, labels, count):
            if t is not None and t.device != self.device:
                raise CavpError(f"ClipValidation lives on {self.device}, got a tensor on {t.device}")
        ops.clipval_update(pred.detach(), is_mask, labels, count, B, T, c, HW, self.num_classes, self.ignore_index, self.min_count,
                           self.min_values, self._hist, self._conf, self._flags, self._counts, self._frames, self._state)

    # ---- reading -----------------------------------------------------------------------------------------------------------
    def counts(self) -> torch.Tensor:
        """int64 [2, K+1, K] (ALL, MS) on the device; zeros on the CPU before the first update."""
        if self._counts is None:
            return torch.zeros((2, self.num_classes + 1, self.num_classes), dtype=torch.int64)
        return self._counts

    def frames(self):
        """(frames counted into ALL, frames counted into MS) as Python ints: one host read."""
        if self._counts is None:
            return 0, 0
        a, m = self._frames.cpu().tolist()
        return a, m

    def results(self, class_list=None):
        """((mIoU, acc, fdr, f1, f0.3) of ALL, the same of MS): get_performance(all_miou, all_fg, class_list) and
        get_performance(ms_miou, ms_fg, class_list) from ONE host copy of the counts."""
        M = self.counts().cpu().numpy()
        k = self.num_classes
        out = []
        for m in M:
            _, _, iou, acc = iou_and_accuracy(m)
            out.append((*pixel_scores(iou, acc, class_list), *detection_scores(torch.tensor(m[:k].astype(numpy.float64)), class_list)))
        return tuple(out)

    def reset(self) -> None:
        """Zero both matrices and the frame counters (the bad-input counters stay until check())."""
        if self._counts is not None:
            _zero_(self._counts)
            _zero_(self._frames)

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, a label was >= 256, a mask byte >= num_classes or a count
        outside [0, T]."""
        if self._counts is None:
            raise CavpError("check: no ClipValidation update yet")
        bad = self._state.cpu().tolist()
        if any(bad[:3]):
            _zero_(self._state)
            raise CavpError(f"ClipValidation: {bad[0]} label(s) >= 256, {bad[1]} mask value(s) >= {self.num_classes}, "
                            f"{bad[2]} count(s) outside [0, T] since the last check")


MAX_VIDEOS = 1 << 20               # per-video slots one VideoValidation may ask for


class VideoValidation:
    """The validation loop of the AVSBench object trainer (S4 / MS3: trainer_cavp_avs_obj.py:292-363) for whole batches of videos,
    without the host:

        vv = VideoValidation(num_classes=2, ignore_index=255, pr_num=255, channel=1, max_frames=320, max_videos=4096)
        vv.update(model(image, audio, eval_mode=True)[0], labels, count)        # or vv.update_lowres(model.predict_lowres(...), ...)
        (avs_miou, avs_f), (miou, acc, fdr, f1, f03) = vv.results()

    logits: dense float32 [B*T, C, H, W], 2 <= C <= num_classes.  labels: dense int64 [B, T, H, W] (or [N, H, W] with count=None:
    one video); never written.  count: device int32 / int64 [B], the reference's mask_num per video: frame t of video b takes part
    iff t < count[b] (None: every frame); a frame that takes no part is not read by the metric kernels.  The reference defines this
    loop only for mask_num == T (its mask_iou asserts equal shapes of the mask_num predictions and the T labels); count[b] < T
    means the reference applied to the first count[b] frames of video b.

    Per video with at least one frame, in float32 with the reference's operations and order: J = mask_iou(argmax(logits), labels)
    (an empty target scores its background overlap over all pixels) and F = Eval_Fmeasure(softmax(logits)[:, channel], labels) (the
    best of `pr_num` thresholds; frames with an all-zero gt are skipped, a video of such frames scores 0; gt = labels != 0), stored
    in the video's slot: batch order within an update, call order across updates.  Every participating frame also adds its
    confusion counts (the (K+1) x K bin rule of MIoU / ForegroundDetect) to one matrix, which `miou` and `fg` read (no copies).

    update() is two launches and update_lowres() three (csrc/metrics.hip); neither synchronises, neither allocates
    after its first call, so both can be captured in a hipGraph with the eval forward (run one eager call first).  The counts are
    integer adds and the float tail runs in a fixed order: the results do not depend on arrival order.  A count[b] outside [0, T]
    is clamped, a video beyond `max_videos` is not stored, a label outside {0, 1, ignore_index} is counted by the rules above all
    the same; each is counted on the device, and check() raises if there were any."""

    def __init__(self, num_classes: int = 2, ignore_index=255, pr_num: int = 255, channel: int = 1, max_frames: int = 320,
                 max_videos: int = 4096, device=None):
        k = int(num_classes)
        if not 2 <= k <= MAX_CLASSES:
            raise CavpError(f"VideoValidation: 2 <= num_classes <= {MAX_CLASSES}, got {num_classes}")
        if not 1 <= int(pr_num) <= ops.VIDEOVAL_MAX_THRESHOLDS:
            raise CavpError(f"VideoValidation: 1 <= pr_num <= {ops.VIDEOVAL_MAX_THRESHOLDS}, got {pr_num}")
        if not 0 <= int(channel) < k:
            raise CavpError(f"VideoValidation: 0 <= channel < num_classes, got {channel}")
        if not 1 <= int(max_frames) <= MAX_CLIP_FRAMES:
            raise CavpError(f"VideoValidation: 1 <= max_frames <= {MAX_CLIP_FRAMES}")
        if not 1 <= int(max_videos) <= MAX_VIDEOS:
            raise CavpError(f"VideoValidation: 1 <= max_videos <= {MAX_VIDEOS}")
        self.num_classes, self.ignore_index = k, ignore_index
        self.pr_num, self.channel, self.max_frames, self.max_videos = int(pr_num), int(channel), int(max_frames), int(max_videos)
        self.nbins = (k + 1) * k
        self._kernel_ignore = -1 if ignore_index is None else int(ignore_index)   # -1 is never counted anyway (t >= 0)
        self._device = device
        self._res = None             # device buffers, allocated by the first update (the constructor touches no device)
        self._lowres = {}            # (N, H, W) -> (mask, prob) of update_lowres
        self.miou = MIoU(k, ignore_index, 0)
        self.fg = ForegroundDetect(k, ignore_index, 0)

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _bind(self, res, stats, hist, th):
        """Take the device buffers.  res int64 [(K+1)K + 8 + max_videos]: the confusion counts, the state words and J | F (float32)
        side by side, so that results() is one host read; stats int64 [max_frames, 4] and hist int32 [max_frames, 2, pr_num + 1]
        (zero at rest); th the threshold table."""
        mf, mv, nb = self.max_frames, self.max_videos, self.nbins
        want = ((res, torch.int64, nb + ops.VIDEOVAL_STATE_WORDS + mv), (stats, torch.int64, 4 * mf),
                (hist, torch.int32, mf * 2 * (self.pr_num + 1)), (th, torch.float32, self.pr_num))
        for t, dt, numel in want:
            if t.dtype != dt or t.numel() != numel or not t.is_contiguous() or not t.is_cuda or t.device != res.device:
                raise CavpError("VideoValidation: device buffers of the wrong dtype, size or device")
        self.device = res.device
        self._res, self._stats, self._hist, self._th = res, stats, hist, th
        self._counts = res[:nb]
        self._state = res[nb:nb + ops.VIDEOVAL_STATE_WORDS]
        scores = res[nb + ops.VIDEOVAL_STATE_WORDS:].view(torch.float32)
        self._J, self._F = scores[:mv], scores[mv:]
        self.miou._adopt(self._counts)
        self.fg._adopt(self._counts)

    def _ensure(self):
        if self._res is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise CavpError("VideoValidation lives on a HIP device (there is no CPU fallback)")
            if torch.cuda.is_current_stream_capturing():
                raise CavpError("VideoValidation would allocate during hipGraph capture; run one eager update first")
            mf = self.max_frames
            self._bind(_zeros((self.nbins + ops.VIDEOVAL_STATE_WORDS + self.max_videos,), torch.int64, dev),
                       _zeros((mf, 4), torch.int64, dev), _zeros((mf, 2, self.pr_num + 1), torch.int32, dev),
                       thresholds(self.pr_num, dev))

    # ---- the updates -------------------------------------------------------------------------------------------------------
    def _check_labels(self, labels, count):
        """(B, T, H, W) of the labels and the optional count."""
        E = CavpError
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() not in (3, 4):
            raise E(f"VideoValidation: labels must be an int64 tensor [B, T, H, W] (or [N, H, W] without count), got "
                    f"{getattr(labels, 'dtype', type(labels))} {tuple(getattr(labels, 'shape', ()))}")
        if labels.dim() == 3 and count is not None:
            raise E("VideoValidation: count needs labels [B, T, H, W]")
        B, T = (labels.shape[0], labels.shape[1]) if labels.dim() == 4 else (1, labels.shape[0])
        H, W = labels.shape[-2:]
        if B * T < 1 or H < 1 or W < 1:
            raise E("VideoValidation: empty labels are not supported")
        if B * T > self.max_frames:
            raise E(f"VideoValidation: {B * T} frames in one update, max_frames = {self.max_frames}")
        if count is not None:
            if not isinstance(count, torch.Tensor) or count.dtype not in (torch.int32, torch.int64) or tuple(count.shape) != (B,):
                raise E(f"VideoValidation: count must be an int32 or int64 tensor of shape ({B},)")
        if not labels.is_contiguous() or (count is not None and not count.is_contiguous()):
            raise E("VideoValidation: dense (contiguous) tensors required")
        return B, T, H, W

    def _on_device(self, *ts):
        for t in ts:
            if t is not None and t.device != self.device:
                raise CavpError(f"VideoValidation lives on {self.device}, got a tensor on {t.device}")

    def _launch(self, pred, prob, labels, count, B, T, hw):
        ops.videoval_frame_stats(pred, labels, count, T, self.num_classes, self._kernel_ignore, self._th, self._stats, self._hist,
                                 self._counts, self._state, self.channel, prob)
        ops.videoval_combine(self._stats, self._hist, count, B, T, hw, self.pr_num, self._J, self._F, self._state)

    def update(self, logits: torch.Tensor, labels: torch.Tensor, count=None) -> None:
        """Score one batch of videos from full-resolution logits (see the class docstring): two launches, no host sync; graph
        replays of a captured update() accumulate the same way."""
        B, T, H, W = self._check_labels(labels, count)
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 4 \
                or logits.shape[0] != B * T or tuple(logits.shape[2:]) != (H, W):
            raise CavpError(f"VideoValidation: float32 logits [{B * T}, C, {H}, {W}] required, got "
                            f"{getattr(logits, 'dtype', type(logits))} {tuple(getattr(logits, 'shape', ()))}")
        c = logits.shape[1]
        if not 2 <= c <= self.num_classes:
            raise CavpError(f"VideoValidation: 2 <= logit channels <= num_classes {self.num_classes}, got {c}")
        if not self.channel < c:
            raise CavpError(f"VideoValidation: channel {self.channel} outside the {c} logit channels")
        if not logits.is_contiguous():
            raise CavpError("VideoValidation: dense (contiguous) tensors required")
        ops._need_gpu(logits, labels, count)
        self._ensure()
        self._on_device(logits, labels, count)
        self._launch(logits.detach(), None, labels, count, B, T, H * W)

    def update_lowres(self, lo: torch.Tensor, labels: torch.Tensor, count=None, input_shape=None, align_corners: bool = False) -> None:
        """update() from the low-resolution logits `lo` (NHWC view [B*T, h, w, C], f32 or bf16: CAVP.predict_lowres): the scores and
        counts of update(full_res_logits, ...) where full_res_logits is the bilinear upsample of `lo` to `input_shape` (default
        labels.shape[-2:]), which is never materialised: ops.seg_predict writes the uint8 class mask and the float32 probability
        plane of all B*T frames, the frame kernel reads those of the participating ones.  Three launches, no host sync, no
        allocation after the first call with a given (B*T, H, W)."""
        B, T, H, W = self._check_labels(labels, count)
        if not isinstance(lo, torch.Tensor) or lo.dim() != 4 or lo.shape[0] != B * T or lo.dtype not in (torch.float32, torch.bfloat16):
            raise CavpError(f"VideoValidation: low-res logits [{B * T}, h, w, C] (float32 or bfloat16) required, got "
                            f"{getattr(lo, 'dtype', type(lo))} {tuple(getattr(lo, 'shape', ()))}")
        shape = (H, W) if input_shape is None else tuple(int(v) for v in input_shape)
        if shape != (H, W):
            raise CavpError(f"VideoValidation: input_shape {shape} differs from the labels' {(H, W)}")
        c = lo.shape[3]
        if not 2 <= c <= min(self.num_classes, 256):
            raise CavpError(f"VideoValidation: 2 <= logit channels <= num_classes {self.num_classes} (and 256: a byte mask), got {c}")
        if not self.channel < c:
            raise CavpError(f"VideoValidation: channel {self.channel} outside the {c} logit channels")
        ops._need_gpu(lo, labels, count)
        self._ensure()
        self._on_device(lo, labels, count)
        key = (B * T, H, W)
        if key not in self._lowres:
            if torch.cuda.is_current_stream_capturing():
                raise CavpError("VideoValidation.update_lowres would allocate during hipGraph capture; run one eager call first")
            self._lowres[key] = (torch.empty(key, dtype=torch.uint8, device=self.device),
                                 torch.empty(key, dtype=torch.float32, device=self.device))
        mask, prob = self._lowres[key]
        ops.seg_predict(lo.detach(), shape, mask=mask, prob=prob, channel=self.channel, align_corners=align_corners)
        self._launch(mask, prob, labels, count, B, T, H * W)

    # ---- reading -----------------------------------------------------------------------------------------------------------
    def counts(self) -> torch.Tensor:
        """The (K+1) x K confusion counts (int64, on the device; zeros on the CPU before the first update)."""
        k = self.num_classes
        if self._res is None:
            return torch.zeros((k + 1, k), dtype=torch.int64)
        return self._counts.view(k + 1, k)

    def _read(self):
        """(M int64 [K+1, K], state [8], J float32 [n], F float32 [n]) on the host from ONE copy of the device buffer."""
        k, nb, mv = self.num_classes, self.nbins, self.max_videos
        if self._res is None:
            empty = numpy.zeros(0, dtype=numpy.float32)
            return numpy.zeros((k + 1, k), dtype=numpy.int64), [0] * ops.VIDEOVAL_STATE_WORDS, empty, empty
        host = self._res.cpu()
        state = host[nb:nb + ops.VIDEOVAL_STATE_WORDS].tolist()
        scores = host[nb + ops.VIDEOVAL_STATE_WORDS:].view(torch.float32).numpy()
        n = min(state[4], mv)
        return host[:nb].numpy().reshape(k + 1, k), state, scores[:n], scores[mv:mv + n]

    def videos(self) -> int:
        """Videos scored so far (those beyond max_videos not included): one host read."""
        return 0 if self._res is None else min(int(self._state[4].item()), self.max_videos)

    def video_scores(self):
        """(J, F): float32 [n] device tensors, one entry per scored video in slot order (views; one host read for n)."""
        if self._res is None:
            empty = torch.zeros(0, dtype=torch.float32)
            return empty, empty
        n = self.videos()
        return self._J[:n], self._F[:n]

    @staticmethod
    def _means(J: numpy.ndarray, F: numpy.ndarray):
        """The reference's two AverageMeter means as Python floats: J (0-d float32 tensors there) summed in float32 in slot order and
        divided in float32, F (Python floats there) summed and divided in double."""
        n = J.shape[0]
        j_mean = numpy.float32(numpy.cumsum(J, dtype=numpy.float32)[-1]) / numpy.float32(n)
        f_sum = 0.0
        for v in F.tolist():
            f_sum += v
        return float(j_mean), f_sum / n

    def video_means(self):
        """(mean J, mean F) before rounding, as Python floats: one host read."""
        _, _, J, F = self._read()
        if J.shape[0] == 0:
            raise CavpError("VideoValidation: no video counted yet (the reference divides by zero here)")
        return self._means(J, F)

    def results(self, class_list=None):
        """((avs_miou, avs_f), (mIoU, acc, fdr, f1, f0.3)) from ONE host read: the means of the per-video J and F in the reference's
        AverageMeter arithmetic, each numpy.round(x, 4) (trainer_cavp_avs_obj.py:349-352), and get_performance(miou, fg, class_list)
        of the frames' confusion counts.  Raises CavpError when no video has been counted (the reference divides by zero)."""
        M, _, J, F = self._read()
        if J.shape[0] == 0:
            raise CavpError("VideoValidation: no video counted yet (the reference divides by zero here)")
        j_mean, f_mean = self._means(J, F)
        k = self.num_classes
        _, _, iou, acc = iou_and_accuracy(M)
        perf = (*pixel_scores(iou, acc, class_list), *detection_scores(torch.tensor(M[:k].astype(numpy.float64)), class_list))
        return (numpy.round(j_mean, 4), numpy.round(f_mean, 4)), perf

    def reset(self) -> None:
        """Forget the videos and zero the confusion counts (the bad-input counters stay until check())."""
        if self._res is not None:
            _zero_(self._counts)
            _zero_(self._state[4:5])

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, a count was outside [0, T], a video was dropped for
        max_videos, a label was outside {0, 1, ignore_index} or a mask byte was >= num_classes."""
        if self._res is None:
            raise CavpError("check: no VideoValidation update yet")
        bad = self._state[:4].cpu().tolist()
        if any(bad):
            _zero_(self._state[:4])
            raise CavpError(f"VideoValidation: {bad[0]} label(s) outside {{0, 1, {self.ignore_index}}}, {bad[1]} mask value(s) >= "
                            f"{self.num_classes}, {bad[2]} count(s) outside [0, T], {bad[3]} video(s) beyond max_videos = "
                            f"{self.max_videos} since the last check")


class SemanticValidation:
    """The AVSBench-semantic metric (utils/avsbench_metrics.py: calc_color_miou_fscore, calc_color_miou, calc_binary_miou; the
    reference's README calls it "Instance-level Evaluation") for whole batches of clips, without the host:

        sv = SemanticValidation(num_classes=K, max_frames=320, device="cuda:0")
        sv.update(model.predict(image, audio), labels, count)            # or sv.update_lowres(model.predict_lowres(...), ...)
        r = sv.results()                                                 # r["miou"], r["fscore"], r["jf"], r["binary_miou"], ...

    pred: dense float32 logits [B*T, K, H, W] (exactly K channels; argmax: first maximal index, a NaN is the maximum; the
    reference's softmax in front of the argmax does not change it and is not computed), or the dense uint8 class mask [B*T, H, W] of
    CAVP.predict.  labels: dense int64 [B, T, H, W] (or [N, H, W] with count=None); never written.  count: device int32 / int64 [B],
    the reference's mask_num per clip: frame t of clip b takes part iff t < clamp(count[b], 0, T) (None: every frame); a frame that
    takes no part is not read.

    Per participating frame, three integer vectors over the classes: inter[c] = #(p == c and l == c), pred[c] = #(p == c and l >= 0),
    lab[c] = #(l == c) - the reference's three torch.histc(bins=K, min=1, max=K) areas.  A pixel with l < 0 counts nowhere; a pixel
    with l >= K (the ignore value 255 included) counts in pred only: the reference's histc drops the label and keeps the
    prediction, and that quirk is kept.  From them in float32, one IEEE operation at a time, in the reference's grouping: iou =
    inter / (2.22e-16 + union), f = 1.3 precision recall / (0.3 precision + recall) (NaN -> 0), hit = (union != 0), and the frame's
    mean IoU over the classes with a non-zero IoU (NaN when there is none, as in the reference).  Within one update the per-class
    sums of iou, f and hit start from zero and take the frames in ascending (b, t): exactly what one call of calc_color_miou_fscore
    returns (last_call()).  The call's sums are then added to the running float32 accumulators, as the benchmark driver's
    `miou_pc += _miou_pc` does (accumulators()).  The binary IoU of calc_binary_miou (foreground = class != 0, over all pixels; an
    empty target scores its background overlap) accumulates the same way.

    results() = the published benchmark driver's reduction: miou_pc = ious / cls_count and fscore_pc = fscores / cls_count (NaN ->
    0), their means over all K classes, jf = (miou + fscore) / 2, binary_miou = binary_sum / frames, in float32 torch operations
    from ONE host copy.  That driver is not part of the reference tree, so this last step is pinned by the restatement
    tests/_semval_ref.py only; everything up to the accumulators is held to the reference's own functions by
    tests/golden/semval.npz.  The label-vocabulary remapping of the benchmark's v1s / v1m / v2 subsets is the caller's.

    update() is two launches and update_lowres() three (csrc/metrics.hip); neither synchronises, neither allocates
    after its first call, so both can be captured in a hipGraph with CAVP.predict / predict_lowres (run one eager call first).  The
    counts are integer adds and the float tail runs in a fixed order, one thread per class: the results do not depend on arrival
    order.  A mask byte >= K sets no class counter, a count[b] outside [0, T] is clamped; each is counted on the device, and check()
    raises if there were any.  The accumulators are per process: summing them across ranks is the caller's job (float32 adds, in a
    rank order of the caller's choice)."""

    def __init__(self, num_classes: int, max_frames: int = 320, device=None):
        k = int(num_classes)
        if not 2 <= k <= MAX_CLASSES:
            raise CavpError(f"SemanticValidation: 2 <= num_classes <= {MAX_CLASSES}, got {num_classes} (one class is degenerate in "
                            f"the reference's histc)")
        if not 1 <= int(max_frames) <= MAX_CLIP_FRAMES:
            raise CavpError(f"SemanticValidation: 1 <= max_frames <= {MAX_CLIP_FRAMES}")
        self.num_classes, self.max_frames = k, int(max_frames)
        self.words = 3 * k + 4
        self.scratch_bytes = self.max_frames * self.words * 4   # at most 3.2 GB (K = 4096, 65535 frames); 72 KB at K = 71, 80 frames
        self._device = device
        self._res = None             # device buffers, allocated by the first update (the constructor touches no device)
        self._lowres = {}            # (N, H, W) -> mask of update_lowres
        self._last_frames = 0

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _bind(self, res, scratch, last):
        """Take the device buffers.  res int64 [4 + ceil((3K + 1) / 2)]: the state words and the float32 accumulators ious | fscores
        | cls_count | binary_sum side by side, so that results() is one host read; scratch int32 [max_frames, 3K + 4] (zero at
        rest); last float32 [3K + 1 + 2 * max_frames]: the last call's sums, frame_miou and the frames' binary IoU."""
        k, mf = self.num_classes, self.max_frames
        sw = ops.SEMVAL_STATE_WORDS
        want = ((res, torch.int64, sw + (3 * k + 2) // 2), (scratch, torch.int32, mf * self.words),
                (last, torch.float32, 3 * k + 1 + 2 * mf))
        for t, dt, numel in want:
            if t.dtype != dt or t.numel() != numel or not t.is_contiguous() or not t.is_cuda or t.device != res.device:
                raise CavpError("SemanticValidation: device buffers of the wrong dtype, size or device")
        self.device = res.device
        self._res, self._scratch, self._last = res, scratch, last
        self._state = res[:sw]
        self._acc = res[sw:].view(torch.float32)[:3 * k + 1]

    def _ensure(self):
        if self._res is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise CavpError("SemanticValidation lives on a HIP device (there is no CPU fallback)")
            if torch.cuda.is_current_stream_capturing():
                raise CavpError("SemanticValidation would allocate during hipGraph capture; run one eager update first")
            k, mf = self.num_classes, self.max_frames
            self._bind(_zeros((ops.SEMVAL_STATE_WORDS + (3 * k + 2) // 2,), torch.int64, dev), _zeros((mf, self.words), torch.int32, dev),
                       _zeros((3 * k + 1 + 2 * mf,), torch.float32, dev))

    # ---- the updates -------------------------------------------------------------------------------------------------------
    def _check_labels(self, labels, count):
        """(B, T, H, W) of the labels and the optional count."""
        E = CavpError
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() not in (3, 4):
            raise E(f"SemanticValidation: labels must be an int64 tensor [B, T, H, W] (or [N, H, W] without count), got "
                    f"{getattr(labels, 'dtype', type(labels))} {tuple(getattr(labels, 'shape', ()))}")
        if labels.dim() == 3 and count is not None:
            raise E("SemanticValidation: count needs labels [B, T, H, W]")
        B, T = (labels.shape[0], labels.shape[1]) if labels.dim() == 4 else (1, labels.shape[0])
        H, W = labels.shape[-2:]
        if B * T < 1 or H < 1 or W < 1:
            raise E("SemanticValidation: empty labels are not supported")
        if B * T > self.max_frames:
            raise E(f"SemanticValidation: {B * T} frames in one update, max_frames = {self.max_frames}")
        if count is not None:
            if not isinstance(count, torch.Tensor) or count.dtype not in (torch.int32, torch.int64) or tuple(count.shape) != (B,):
                raise E(f"SemanticValidation: count must be an int32 or int64 tensor of shape ({B},)")
        if not labels.is_contiguous() or (count is not None and not count.is_contiguous()):
            raise E("SemanticValidation: dense (contiguous) tensors required")
        return B, T, H, W

    def _launch(self, pred, is_mask, labels, count, B, T, c, hw):
        self._ensure()
        for t in (pred, labels, count):
            if t is not None and t.device != self.device:
                raise CavpError(f"SemanticValidation lives on {self.device}, got a tensor on {t.device}")
        ops.semval_update(pred, is_mask, labels, count, B, T, c, hw, self.num_classes, self.max_frames, self._scratch, self._acc,
                          self._last, self._state)
        self._last_frames = B * T

    def update(self, pred: torch.Tensor, labels: torch.Tensor, count=None) -> None:
        """Score one batch of clips (see the class docstring): two launches, no host sync; graph replays of a captured update()
        accumulate the same way."""
        B, T, H, W = self._check_labels(labels, count)
        N, k = B * T, self.num_classes
        if not isinstance(pred, torch.Tensor):
            raise CavpError("SemanticValidation: pred is a tensor")
        is_mask = pred.dtype == torch.uint8
        if is_mask:
            if tuple(pred.shape) != (N, H, W):
                raise CavpError(f"SemanticValidation: a uint8 class mask of shape {(N, H, W)} required, got {tuple(pred.shape)}")
            c = 0
        elif pred.dtype == torch.float32:
            if pred.dim() != 4 or pred.shape[0] != N or tuple(pred.shape[2:]) != (H, W):
                raise CavpError(f"SemanticValidation: float32 logits [{N}, {k}, {H}, {W}] required, got {tuple(pred.shape)}")
            c = pred.shape[1]
            if c != k:
                raise CavpError(f"SemanticValidation: the logits have {c} channels, num_classes is {k}: the metric takes its class "
                                f"number from the logits")
        else:
            raise CavpError(f"SemanticValidation: pred is a uint8 class mask [N, H, W] or float32 logits [N, K, H, W], got {pred.dtype}")
        if not pred.is_contiguous():
            raise CavpError("SemanticValidation: dense (contiguous) tensors required")
        ops._need_gpu(pred, labels, count)
        self._launch(pred.detach(), is_mask, labels, count, B, T, c, H * W)

    def update_lowres(self, lo: torch.Tensor, labels: torch.Tensor, count=None, input_shape=None, align_corners: bool = False) -> None:
        """update() from the low-resolution logits `lo` (NHWC view [B*T, h, w, K], f32 or bf16: CAVP.predict_lowres): the result of
        update(full_res_logits, ...), bit for bit, where full_res_logits is the bilinear upsample of `lo` to `input_shape` (default
        labels.shape[-2:]), which is never materialised: ops.seg_predict writes the uint8 class mask of all B*T frames, the frame
        kernel reads the participating ones.  K <= 256 (a byte mask).  Three launches, no host sync, no allocation after the first
        call with a given (B*T, H, W)."""
        B, T, H, W = self._check_labels(labels, count)
        if not isinstance(lo, torch.Tensor) or lo.dim() != 4 or lo.shape[0] != B * T or lo.dtype not in (torch.float32, torch.bfloat16):
            raise CavpError(f"SemanticValidation: low-res logits [{B * T}, h, w, K] (float32 or bfloat16) required, got "
                            f"{getattr(lo, 'dtype', type(lo))} {tuple(getattr(lo, 'shape', ()))}")
        shape = (H, W) if input_shape is None else tuple(int(v) for v in input_shape)
        if shape != (H, W):
            raise CavpError(f"SemanticValidation: input_shape {shape} differs from the labels' {(H, W)}")
        c = lo.shape[3]
        if c != self.num_classes or c > 256:
            raise CavpError(f"SemanticValidation: the low-res logits have {c} channels, num_classes is {self.num_classes} (and at "
                            f"most 256: a byte mask)")
        ops._need_gpu(lo, labels, count)
        self._ensure()
        if lo.device != self.device:
            raise CavpError(f"SemanticValidation lives on {self.device}, got a tensor on {lo.device}")
        key = (B * T, H, W)
        if key not in self._lowres:
            if torch.cuda.is_current_stream_capturing():
                raise CavpError("SemanticValidation.update_lowres would allocate during hipGraph capture; run one eager call first")
            self._lowres[key] = torch.empty(key, dtype=torch.uint8, device=self.device)
        mask = self._lowres[key]
        ops.seg_predict(lo.detach(), shape, mask=mask, align_corners=align_corners)
        self._launch(mask, True, labels, count, B, T, 0, H * W)

    # ---- reading -----------------------------------------------------------------------------------------------------------
    def accumulators(self) -> torch.Tensor:
        """float32 [3, K] on the device: ious | fscores | cls_count, the running sums over all updates (a view; zeros on the CPU
        before the first update)."""
        k = self.num_classes
        if self._res is None:
            return torch.zeros((3, k), dtype=torch.float32)
        return self._acc[:3 * k].view(3, k)

    def last_call(self):
        """(ious [K], fscores [K], cls_count [K], frame_miou [N]) of the last update as float32 device views: what one call of the
        reference's calc_color_miou_fscore on that batch returns.  frame_miou reads -1 for a frame that took no part."""
        if self._res is None:
            raise CavpError("last_call: no SemanticValidation update yet")
        k = self.num_classes
        return (self._last[:k], self._last[k:2 * k], self._last[2 * k:3 * k], self._last[3 * k + 1:3 * k + 1 + self._last_frames])

    def frames(self) -> int:
        """Frames scored so far: one host read."""
        return 0 if self._res is None else int(self._state[2].item())

    @staticmethod
    def _finish(ious: torch.Tensor, fscores: torch.Tensor, cls_count: torch.Tensor, binary_sum: torch.Tensor, frames: int) -> dict:
        """The benchmark driver's reduction of the float32 host accumulators (see the class docstring)."""
        if frames < 1:
            raise CavpError("SemanticValidation: no frame counted yet")
        miou_pc, fscore_pc = ious / cls_count, fscores / cls_count
        miou_pc[miou_pc != miou_pc] = 0
        fscore_pc[fscore_pc != fscore_pc] = 0
        miou, fscore = miou_pc.mean(), fscore_pc.mean()
        binary = binary_sum / torch.tensor(frames, dtype=torch.float32)
        return {"miou": miou.item(), "fscore": fscore.item(), "jf": ((miou + fscore) / 2).item(), "binary_miou": binary.item(),
                "miou_pc": miou_pc, "fscore_pc": fscore_pc, "cls_count": cls_count.clone()}

    def results(self) -> dict:
        """{"miou", "fscore", "jf", "binary_miou"} as Python floats and {"miou_pc", "fscore_pc", "cls_count"} as float32 [K] host
        tensors, from ONE host copy.  Raises CavpError when no frame has been counted."""
        if self._res is None:
            raise CavpError("SemanticValidation: no frame counted yet")
        host = self._res.cpu()
        k, sw = self.num_classes, ops.SEMVAL_STATE_WORDS
        acc = host[sw:].view(torch.float32)
        return self._finish(acc[:k], acc[k:2 * k], acc[2 * k:3 * k], acc[3 * k], int(host[2]))

    def reset(self) -> None:
        """Zero the accumulators and the frame counter (the bad-input counters stay until check())."""
        if self._res is not None:
            _zero_(self._res[2:])

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, a mask byte was >= num_classes or a count outside [0, T]."""
        if self._res is None:
            raise CavpError("check: no SemanticValidation update yet")
        bad = self._state[:2].cpu().tolist()
        if any(bad):
            _zero_(self._state[:2])
            raise CavpError(f"SemanticValidation: {bad[0]} mask value(s) >= {self.num_classes}, {bad[1]} count(s) outside [0, T] "
                            f"since the last check")


_semval_private = {}


def _semval_call(pred: torch.Tensor, target: torch.Tensor) -> numpy.ndarray:
    """One update of a private SemanticValidation on (pred [BF, C, H, W] logits, target [BF, H, W]) and ONE host read: the float32
    host copy of its last-call buffer ious | fscores | cls_count | binary sum | frame_miou [BF] | ..."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor) or pred.dim() != 4 or target.dim() != 3:
        raise CavpError("avsbench metrics: pred [BF, C, H, W] logits and target [BF, H, W] required")
    ops._need_gpu(pred, target)
    k, n = pred.shape[1], pred.shape[0]
    key = (k, pred.device)
    sv = _semval_private.get(key)
    if sv is None or sv.max_frames < n:
        sv = _semval_private[key] = SemanticValidation(k, max_frames=max(n, 1), device=pred.device)
    sv.update(pred.float().contiguous(), target.long().contiguous())
    return sv._last.cpu()


def calc_color_miou_fscore(pred, target, T=10):
    """The reference's calc_color_miou_fscore: (ious [C], fscores [C], cls_count [C], vid_miou_list) - the per-class sums of the
    per-frame IoU and F-score (beta^2 = 0.3) over the BF frames and the number of frames each class occurs in, as float32 host
    tensors, and the list of the BF per-frame mean IoUs (0-d float32 host tensors).  pred: device logits [BF, C, H, W]; target:
    [BF, H, W] class indices.  T is accepted and unused, as in the reference."""
    host = _semval_call(pred, target)
    k, n = pred.shape[1], pred.shape[0]
    return host[:k].clone(), host[k:2 * k].clone(), host[2 * k:3 * k].clone(), list(host[3 * k + 1:3 * k + 1 + n].clone().unbind(0))


def calc_color_miou(pred, target, T=10):
    """The reference's calc_color_miou: (ious [C], cls_count [C]) of calc_color_miou_fscore."""
    host = _semval_call(pred, target)
    k = pred.shape[1]
    return host[:k].clone(), host[2 * k:3 * k].clone()


def calc_binary_miou(pred, target, eps=1e-7, size_average=True):
    """The reference's calc_binary_miou: the mean over the N frames of the IoU of (argmax != 0) against (target != 0), an empty
    target scoring its background overlap over all pixels, as a 0-d float32 host tensor.  eps is fixed at the default 1e-7;
    size_average is accepted and unused, as in the reference."""
    if eps != 1e-7:
        raise CavpError("calc_binary_miou: eps is fixed at 1e-7 on the device")
    host = _semval_call(pred, target)
    return host[3 * pred.shape[1]] / torch.tensor(pred.shape[0], dtype=torch.float32)
