"""numpy restatement of the gradient accumulator's rules (cavp_amd/accumulate.py, struct cavp_accum_state): the window's f32 sum
in micro-step order, the k / gate sequence, the loss sums and window means, and the record sequence of an accumulating run.
Shared by test_accumulate_host.py (against torch's .grad accumulation) and test_gpu_accumulate.py (against the kernels)."""
import numpy as np

F32 = np.float32


def window_sum(grads):
    """The arena after the closing micro-step: ((g0 + g1) + g2) + ..., one IEEE f32 add per element and micro-step.  grads: the
    per-micro-step f32 gradients of one window, in order.  One micro-step: the gradient itself, untouched."""
    acc = np.array(grads[0], dtype=F32, copy=True)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in grads[1:]:
            acc = (acc + np.asarray(g, dtype=F32)).astype(F32)
    return acc


def accumulator_after(grads_so_far):
    """The accumulator after a micro-step that did not close its window: a copy of g0 after k = 0, the running sum afterwards."""
    return window_sum(grads_so_far)


def gate_sequence(n, steps, k0=0):
    """[(k, gate)] of `steps` micro-steps from k = k0: k is the micro-step's index in its window, gate whether it closes it."""
    out, k = [], k0
    for _ in range(steps):
        gate = int(k == n - 1)
        out.append((k, gate))
        k = 0 if gate else k + 1
    return out


def loss_sum(losses):
    """sum <- (k == 0 ? l : sum + l) in f32, in micro-step order."""
    s = F32(losses[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for l in losses[1:]:
            s = F32(s + F32(l))
    return s


def window_mean(losses):
    """sum / N, correctly rounded to f32: numpy's f32 division is IEEE, and N is exact in f32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(loss_sum(losses) / F32(len(losses)))


def window_mean_via_float64(losses):
    """The same quotient formed in float64 and rounded once more: 53 >= 2 * 24 + 2 bits, so the double rounding is innocuous and
    this equals window_mean bit for bit (test_accumulate_host.py checks it)."""
    return F32(np.float64(loss_sum(losses)) / np.float64(len(losses)))


def record_sequence(n, micro_skips, lr_of_step):
    """The records of an accumulating run.  micro_skips[i]: whether the window that micro-step i closes is skipped by the guard
    (ignored for micro-steps that close nothing).  Only closing micro-steps write a record; a skipped window leaves t alone.
    Returns [(micro-step index, t, lr, skipped)] and the final (t, skipped_total, windows, k)."""
    t, skipped_total, windows, out = 0, 0, 0, []
    seq = gate_sequence(n, len(micro_skips))
    for i, ((k, gate), s) in enumerate(zip(seq, micro_skips)):
        if not gate:
            continue
        windows += 1
        out.append((i, t, lr_of_step(t), bool(s)))
        if s:
            skipped_total += 1
        else:
            t += 1
    k_next = 0 if not seq or seq[-1][1] else seq[-1][0] + 1
    return out, (t, skipped_total, windows, k_next)
