"""Float64 restatement of the step guard's rules (include/cavp_hip.h, struct cavp_guard_state): per-tensor sum of squares ->
norms, the clip coefficient, the skip rule and the record sequence.  Shared by test_step_guard_host.py (against torch's
clip_grad_norm_) and test_gpu_step_guard.py (against the kernels).  numpy only."""
import math

import numpy as np

BLOCK = 4096                               # elements per optimiser block: one f32 partial each
F32_MAX = float(np.finfo(np.float32).max)


def tensor_sumsq(g) -> float:
    """Sum of squares of one gradient tensor in float64.  The device keeps one f32 partial per 4096-element block, so a block
    whose sum exceeds the f32 range is +inf there; the same here.  Non-finite elements propagate as they do in IEEE arithmetic."""
    x = np.asarray(g, dtype=np.float64).ravel()
    total = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(0, x.size, BLOCK):
            s = float(np.sum(x[b:b + BLOCK] ** 2))
            total += math.inf if s > F32_MAX else s
    return total


def count_nonfinite(g) -> int:
    return int(np.count_nonzero(~np.isfinite(np.asarray(g, dtype=np.float64))))


def clip_coef(grad_norm: float, max_norm) -> float:
    """torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1); no clipping for max_norm None or <= 0."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = max_norm / (grad_norm + 1e-6)
    return 1.0 if math.isnan(c) else min(1.0, c)   # fmin(1, NaN) = 1


def guard_step(grads, kinds, max_norm=None, skip_nonfinite=True, losses=(), skip_nonfinite_loss=True):
    """One step's fields.  grads: the gradient tensors the update reads, kinds: 0 = SGD, 1 = Adam per tensor.  losses: the recorded
    loss values; with skip_nonfinite_loss (a switch of its own) a loss that is not finite skips as well (`skip_on_loss`)."""
    ss = [0.0, 0.0]
    nonfinite = 0
    for g, k in zip(grads, kinds):
        ss[1 if k else 0] += tensor_sumsq(g)
        nonfinite += count_nonfinite(g)
    norm = math.sqrt(ss[0] + ss[1]) if not math.isnan(ss[0] + ss[1]) else math.nan
    bad = nonfinite > 0 or not math.isfinite(norm)
    on_loss = bool(skip_nonfinite_loss) and any(not math.isfinite(float(x)) for x in losses)
    return dict(grad_norm=norm, norm_sgd=math.sqrt(ss[0]) if ss[0] == ss[0] else math.nan,
                norm_adam=math.sqrt(ss[1]) if ss[1] == ss[1] else math.nan, nonfinite=nonfinite,
                clip_coef=clip_coef(norm, max_norm), skip=(bool(skip_nonfinite) and bad) or on_loss, skip_on_loss=on_loss)


def record_sequence(skips, lr_of_step):
    """The records of a run: skips[i] says whether launch i was skipped.  A skipped step leaves t alone, so the next one runs as
    the same index with the same rate.  Returns [(t, lr, skipped)] and the final (t, skipped_total)."""
    t, skipped_total, out = 0, 0, []
    for s in skips:
        out.append((t, lr_of_step(t), bool(s)))
        if s:
            skipped_total += 1
        else:
            t += 1
    return out, (t, skipped_total)


def ring_read(head: int, history: int, read_head: int):
    """Which records a read() returns (indices into the run, oldest first) and how many were overwritten unread."""
    first = max(read_head, head - history)
    return list(range(first, head)), first - read_head
