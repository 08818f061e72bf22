"""Float64 restatement of the wave stage's rules (include/cavp_hip.h "wave stage", cavp_amd/wave.py): resample with the published
sinc_interp_hann kernel over the WHOLE clip and the FULL 2 * width + o tap table, crop_audio's slice, mean over the channels, sum
over the sources, segment select, bad-input rows.  Independent of the product's compact table and of its window-only evaluation.

torchaudio is not a dependency of this project: the resampler is pinned to this restatement of the published algorithm
(torchaudio.functional._get_sinc_resample_kernel / _apply_sinc_resample_kernel), not to torchaudio's output."""
import math

import numpy as np
import torch

TARGET = 16000
LPW, ROLLOFF = 6, 0.99


def full_kernel(rate):
    """(h float32 [n, 2 * width + o], o, n, width) as Resample(rate, 16000) builds it (dtype=None: float64 table, rounded)."""
    g = math.gcd(int(rate), TARGET)
    o, n = int(rate) // g, TARGET // g
    base_freq = min(o, n) * ROLLOFF
    width = math.ceil(LPW * o / base_freq)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    # `torch.arange(0, -n, -1)[:, None, None] / n`: an int64 tensor by an int divides in the default dtype, float32
    t = (torch.arange(0, -n, -1)[:, None, None].to(torch.float32) / torch.tensor(n, dtype=torch.float32)) + idx
    t *= base_freq
    t = t.clamp_(-LPW, LPW)
    window = torch.cos(t * math.pi / LPW / 2) ** 2
    t *= math.pi
    scale = base_freq / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels.to(torch.float32)[:, 0].numpy(), o, n, width


def target_len(L, rate):
    g = math.gcd(int(rate), TARGET)
    o, n = int(rate) // g, TARGET // g
    return -((-n * int(L)) // o)      # ceil(n * L / o), exact integers


def resample64(x, rate, absolute=False):
    """x [..., L] -> float64 [..., ceil(n L / o)]; absolute=True: the same sum over |h| |x| (the error bound's M)."""
    x = np.asarray(x, dtype=np.float64)
    if int(rate) == TARGET:
        return np.abs(x) if absolute else x.copy()
    h, o, n, width = full_kernel(rate)
    h = h.astype(np.float64)
    if absolute:
        x, h = np.abs(x), np.abs(h)
    L = x.shape[-1]
    xp = np.concatenate([np.zeros(x.shape[:-1] + (width,)), x, np.zeros(x.shape[:-1] + (width + o,))], axis=-1)
    win = np.lib.stride_tricks.sliding_window_view(xp, h.shape[1], axis=-1)[..., ::o, :]      # [..., Q, K], frame q starts at q o
    y = win @ h.T                                                                            # [..., Q, n]: y[q n + p]
    return y.reshape(x.shape[:-1] + (-1,))[..., :target_len(L, rate)]


def resample_conv1d_f32(x, rate):
    """The reference's own float32 path (conv1d over the whole clip), for timing and for the bound's sanity check.  x: [C, L]."""
    x = torch.as_tensor(x, dtype=torch.float32)
    if int(rate) == TARGET:
        return x
    h, o, n, width = full_kernel(rate)
    L = x.shape[-1]
    xp = torch.nn.functional.pad(x, (width, width + o))
    y = torch.nn.functional.conv1d(xp[:, None], torch.from_numpy(h)[:, None], stride=o)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[..., :target_len(L, rate)]


def crop_range(L16, sample_len):
    """(s0, ln) of rule 2."""
    st = L16 // 2 - sample_len // 2
    et = st + sample_len
    s0 = st if st >= 0 else max(L16 + st, 0)
    s1 = min(et, L16)
    return s0, s1 - s0


def crop(y, sample_len):
    """y [..., L16] -> [..., sample_len]."""
    s0, ln = crop_range(y.shape[-1], sample_len)
    i = np.arange(sample_len)
    return y[..., s0 + (i if ln == sample_len else i % ln)]


def crop_audio_literal(y, sample_len):
    """The reference's crop_audio expression on a [C, L] torch tensor (what rule 2 restates)."""
    mid_ = y.shape[1] // 2
    st = mid_ - sample_len // 2
    et = st + sample_len
    y = y[:, st:et]
    if y.shape[1] != sample_len:
        y = y.repeat(1, sample_len // y.shape[1] + 1)[:, :sample_len]
    return y


def wave_ref(raw, length, rate_idx, n_ch, rates, sample_len, segments=1, select=None, absolute=False):
    """Rules 1-5 on host arrays: raw float or int16 [B, S, C, Lmax].  Returns (out float64 [B, 1, A_out], bad count)."""
    raw = np.asarray(raw)
    x_all = raw.astype(np.float64) / 32768.0 if raw.dtype == np.int16 else raw.astype(np.float64)
    B, S, C, Lmax = raw.shape
    A_out = sample_len // segments if select is not None else sample_len
    out = np.zeros((B, 1, A_out))
    bad = 0
    for b in range(B):
        row_bad = 0
        if select is not None and not 0 <= int(select[b]) < segments:
            row_bad += 1
        for s in range(S):
            L = int(length[b, s])
            if not 0 <= L <= Lmax:
                row_bad += 1
            elif L > 0:
                row_bad += not 0 <= int(rate_idx[b, s]) < len(rates)
                row_bad += not 1 <= int(n_ch[b, s]) <= C
        bad += row_bad
        if row_bad:
            continue
        acc = np.zeros(sample_len)
        for s in range(S):
            L = int(length[b, s])
            if L == 0:
                continue
            nc = int(n_ch[b, s])
            y = resample64(x_all[b, s, :nc, :L], rates[int(rate_idx[b, s])], absolute)
            acc += crop(y, sample_len).sum(0) / nc
        out[b, 0] = acc[int(select[b]) * A_out:(int(select[b]) + 1) * A_out] if select is not None else acc
    return out, bad


# ---- the inputs of tests/golden/wave_crop.npz (tools/make_golden_wave.py writes the outputs of the reference's code on them) ----
GOLDEN_SAMPLE_LENS = (400, 16000)
GOLDEN_AUDIO_LEN = {400: 0.025, 16000: 1.0}
GOLDEN_SEGMENTS = 10


def golden_lengths(sample_len):
    """One length per crop regime: 1, below sample_len / 3 (the whole clip repeats), between (the negative start wraps), equal,
    longer."""
    return (1, sample_len // 4, (2 * sample_len) // 3 + 1, sample_len, sample_len + sample_len // 2 + 3)


def golden_input(seed, channels, L):
    """int16 [channels, L], a short period so that the fixture compresses; v / 32768 is exact in float32."""
    i = np.arange(L, dtype=np.int64)[None, :]
    c = np.arange(channels, dtype=np.int64)[:, None]
    return (((i * 37 + c * 11 + seed * 5) % 61 - 30) * 64).astype(np.int16)


def golden_cases(sample_len):
    """name -> (kind, [(seed, channels, L) per source], img_id or None)."""
    Ls = golden_lengths(sample_len)
    cases = {}
    for k, L in enumerate(Ls):
        cases[f"avss_{sample_len}_{k}"] = ("avss", [(k, 2, L)], None)
    for k, (a, b) in enumerate(((1, 4), (2, 3), (0, 2))):
        cases[f"vpo_{sample_len}_{k}"] = ("vpo", [(10 + k, 1, Ls[a]), (20 + k, 1, Ls[b])], None)
    for k, (a, img_id) in enumerate(((2, 1), (4, 7), (3, 10))):
        cases[f"avsb_{sample_len}_{k}"] = ("avsb", [(30 + k, 2, Ls[a])], img_id)
    return cases
