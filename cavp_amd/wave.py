"""Raw audio clips to the model's mono 16 kHz window on the GPU: what every data set of the reference does on the host, per item,
between torchaudio.load and the batch - torchaudio.transforms.Resample(rate, 16000) over the whole file, crop_audio (centre crop to
int(audio_len * 16000) samples, repeat for short clips), torch.stack(wave_list).sum(0) over the sources of a VPO image or
torch.mean(wave, dim=0) over the channels, and for the AVSBench training items view(1, 10, -1)[:, img_id - 1]
(dataset/vpo_mono/multi_source/audio/audio_dataset.py:48-70, dataset/avss/audio/audio_dataset.py:42-62,
dataset/avsbench_ms.py:129-134,156-159,169-180, dataset/avsbench_s4.py:120-149) - as ONE launch of csrc/wave.hip with no host value
that depends on a device value: capturable in a hipGraph in front of PairBuilder and MelFrontEnd.  Only the cropped window of the
resampled signal is computed, not the whole file.

    ws = WaveStage(audio_len=1.0, rates=(16000, 44100, 48000), max_sources=S, max_channels=C, max_len=Lmax, segments=1,
                   device=dev, max_batch=Bmax)
    out = ws(raw, length, rate_idx, n_ch, select=None, out=None)       # out.waveform: f32 [B, 1, A_out]
    pairs = pb(out.waveform, pix_label, img_label, overwrite=...)       # PairBuilder, then MelFrontEnd
    ws.check()                                                          # raises if the device-side bad counter is non-zero

Opt-in and additive: nothing that exists changes.  Inputs (contiguous device tensors, never written): raw float32 or int16
[B, S, C, Lmax] (the staging buffer decoded PCM is copied into; an int16 v stands for v / 32768), length int32 [B, S] (0: the source
is absent), rate_idx int32 [B, S] (index into `rates`), n_ch int32 [B, S] (1 .. C), select int32 [B] (only with segments > 1: the
output is segment select[b] of the window, A_out = sample_len // segments; without it A_out = sample_len and the caller views it as
[B, segments, -1]).  The rules are restated in include/cavp_hip.h ("wave stage"), tests/_wave_ref.py and DESIGN.md 4t.

The resampler is the published sinc_interp_hann kernel (lowpass_filter_width 6, rolloff 0.99) built in float64 the way torchaudio
builds it and rounded to float32; per phase everything outside one contiguous span rounds to exactly 0.0f, so the device holds a
compact [phases, span] table and a first-tap index per phase: the same filter with 13 .. 37 taps instead of up to 475."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

TARGET_RATE = 16000
LOWPASS_WIDTH, ROLLOFF = 6, 0.99
MIN_RATE, MAX_RATE, MAX_RATES = 4000, 192000, 8
MAX_TABLE_BYTES = 64 * 1024
MAX_LDS_BYTES = 160 * 1024
MAX_BATCH, MAX_LEN = 65535, 1 << 28
TILE = 1024        # outputs per workgroup: cavp_wave_tile()


def resample_ratio(rate: int):
    """(o, n, width): the reduced ratio rate : 16000 and the half width of the filter in source samples."""
    g = math.gcd(int(rate), TARGET_RATE)
    o, n = int(rate) // g, TARGET_RATE // g
    base = min(o, n) * ROLLOFF
    return o, n, math.ceil(LOWPASS_WIDTH * o / base)


def _kernel_rows(o: int, n: int, width: int, p0: int, p1: int) -> np.ndarray:
    """Rows p0 .. p1 of the float32 [n, 2 * width + o] filter, with torchaudio's own statements (_get_sinc_resample_kernel with
    dtype=None: float64 sample offsets, the phase offsets -p / n divided in float32 as `int64 tensor / int` does)."""
    base = min(o, n) * ROLLOFF
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, :] / o
    phase = (torch.arange(-p0, -p1, -1, dtype=torch.int64).to(torch.float32) / torch.tensor(float(n), dtype=torch.float32))[:, None]
    t = phase.to(torch.float64) + idx
    t *= base
    t = t.clamp_(-LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels *= window * (base / o)
    return kernels.to(torch.float32).numpy()


def compact_table(rate: int) -> dict:
    """The filter of one rate as the device holds it: taps float32 [n, stride] (the live taps of each phase first, zeros behind;
    stride odd so that adjacent phases start in different LDS banks), first int32 [n] (first live tap of each phase less `fmin`),
    span, and shift = fmin - width.  Raises CavpError when n * stride * 4 exceeds 64 KiB."""
    E = _lib.CavpError
    if rate == TARGET_RATE:
        return {"o": 1, "n": 1, "width": 0, "span": 1, "stride": 1, "taps": np.ones((1, 1), np.float32), "first": np.zeros(1, np.int32),
                "shift": 0, "fspread": 0}
    o, n, width = resample_ratio(rate)
    # no phase has fewer than 12 live taps (the window is 12 / rolloff source samples wide at least): refuse before building rows
    if n * 12 * 4 > MAX_TABLE_BYTES:
        raise E(f"WaveStage: the filter of rate {rate} ({n} phases) exceeds {MAX_TABLE_BYTES} bytes")
    K = 2 * width + o
    rows, lo, hi = [], np.empty(n, np.int64), np.empty(n, np.int64)
    step = max(1, (1 << 22) // K)
    for p0 in range(0, n, step):
        h = _kernel_rows(o, n, width, p0, min(n, p0 + step))
        for i, row in enumerate(h):
            nz = np.flatnonzero(row)
            if nz.size == 0:
                raise E(f"WaveStage: the filter of rate {rate} has an empty phase")
            lo[p0 + i], hi[p0 + i] = nz[0], nz[-1]
            rows.append(row[nz[0]:nz[-1] + 1].copy())
    span = int((hi - lo).max()) + 1
    stride = span | 1
    if n * stride * 4 > MAX_TABLE_BYTES:
        raise E(f"WaveStage: the filter of rate {rate} ({n} phases of {span} taps) exceeds {MAX_TABLE_BYTES} bytes")
    taps = np.zeros((n, stride), np.float32)
    for p, row in enumerate(rows):
        taps[p, :row.size] = row
    fmin = int(lo.min())
    return {"o": o, "n": n, "width": width, "span": span, "stride": stride, "taps": taps, "first": (lo - fmin).astype(np.int32),
            "shift": fmin - width, "fspread": int(lo.max()) - fmin}


class WaveResult:
    """Output of one WaveStage call: waveform f32 [B, 1, A_out] on the device."""
    __slots__ = ("waveform",)

    def __init__(self, B, A_out, dev):
        self.waveform = torch.empty((B, 1, A_out), dtype=torch.float32, device=dev)


class WaveStage:
    """See the module docstring.  Limits: at most 8 rates in [4000, 192000] whose compact filter fits 64 KiB each, B <= max_batch
    <= 65535, max_len <= 2^28 samples, mono output (keeping the channels is out of scope; PairBuilder rejects stereo anyway)."""

    def __init__(self, audio_len: float, rates: Sequence[int], max_sources: int, max_channels: int, max_len: int, segments: int = 1,
                 device=None, max_batch: int = 64):
        E = _lib.CavpError
        rates = tuple(rates)
        if not 1 <= len(rates) <= MAX_RATES:
            raise E(f"WaveStage: 1 .. {MAX_RATES} rates")
        for r in rates:
            if int(r) != r or not MIN_RATE <= int(r) <= MAX_RATE:
                raise E(f"WaveStage: rate {r} is no integer in [{MIN_RATE}, {MAX_RATE}]")
        self.rates = tuple(int(r) for r in rates)
        self.sample_len = int(audio_len * TARGET_RATE)      # the reference's expression, Python's float semantics
        self.segments = int(segments)
        if self.sample_len < 1 or self.segments < 1 or self.sample_len % self.segments:
            raise E(f"WaveStage: sample_len = int(audio_len * 16000) = {self.sample_len} must be positive and divisible by segments")
        if int(max_sources) < 1 or int(max_channels) < 1:
            raise E("WaveStage: max_sources and max_channels must be positive")
        if not 1 <= int(max_len) <= MAX_LEN:
            raise E(f"WaveStage: 1 <= max_len <= {MAX_LEN}")
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise E(f"WaveStage: 1 <= max_batch <= {MAX_BATCH}")
        self.S, self.C, self.Lmax, self.max_batch = int(max_sources), int(max_channels), int(max_len), int(max_batch)
        self.tables = [compact_table(r) for r in self.rates]
        desc, taps, first = [], [], []
        tap_off = first_off = 0
        for tb in self.tables:
            desc.append([tb["o"], tb["n"], tb["span"], tb["stride"], tap_off, first_off, tb["shift"], tb["fspread"]])
            taps.append(tb["taps"].reshape(-1))
            first.append(tb["first"])
            tap_off += tb["taps"].size
            first_off += tb["first"].size
        self.desc_host = np.array(desc, dtype=np.int32)
        self.taps_host = np.concatenate(taps)
        self.first_host = np.concatenate(first)
        # LDS of a workgroup: one rate's filter and first-tap indices, and the input span of one tile of outputs
        self.tab_cap = max(tb["n"] * tb["stride"] for tb in self.tables)
        self.first_cap = max(tb["n"] for tb in self.tables)
        self.x_cap = max(((TILE - 1) // tb["n"] + 1) * tb["o"] + tb["fspread"] + tb["span"] for tb in self.tables)
        if (self.tab_cap + self.first_cap + self.x_cap) * 4 > MAX_LDS_BYTES:
            raise E(f"WaveStage: these rates need {(self.tab_cap + self.first_cap + self.x_cap) * 4} bytes of LDS, more than {MAX_LDS_BYTES}")
        self._device = device
        self._state = None       # device buffers, allocated by the first call (the constructor touches no device)

    # ---- device state ------------------------------------------------------------------------------------------------------
    def _ensure(self):
        if self._state is None:
            dev = torch.device(self._device) if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise _lib.CavpError("WaveStage lives on a HIP device (there is no CPU fallback)")
            if _lib.load().cavp_wave_tile() != TILE:
                raise _lib.CavpError("WaveStage: libcavp_hip.so was built with another output tile; rebuild")
            self.device = dev
            self._desc = torch.from_numpy(self.desc_host).to(dev)
            self._taps = torch.from_numpy(self.taps_host).to(dev)
            self._first = torch.from_numpy(self.first_host).to(dev)
            self._state = torch.zeros(4, dtype=torch.int64, device=dev)       # {bad_inputs, reserved x 3}
        return self._state

    def check(self) -> None:
        """Synchronises and raises CavpError if, since the last check, a length, rate_idx, n_ch or select was out of range (the
        rows they belong to were written as zeros)."""
        if self._state is None:
            raise _lib.CavpError("check: no WaveStage call yet")
        bad = int(self._state[0].item())
        if bad:
            self._state[0:1].zero_()
            raise _lib.CavpError(f"WaveStage: {bad} input value(s) out of range (length, rate_idx, n_ch or select)")

    def out_len(self, select: bool) -> int:
        return self.sample_len // self.segments if select else self.sample_len

    # ---- the call -----------------------------------------------------------------------------------------------------------
    def _check_inputs(self, raw, length, rate_idx, n_ch, select):
        E = _lib.CavpError
        if not isinstance(raw, torch.Tensor) or raw.dtype not in (torch.float32, torch.int16) or raw.dim() != 4:
            raise E("WaveStage: raw must be float32 or int16 [B, S, C, Lmax]")
        B = raw.shape[0]
        if tuple(raw.shape[1:]) != (self.S, self.C, self.Lmax):
            raise E(f"WaveStage: built for raw [B, {self.S}, {self.C}, {self.Lmax}], got {tuple(raw.shape)}")
        if not 1 <= B <= self.max_batch:
            raise E(f"WaveStage: batch {B} outside [1, max_batch = {self.max_batch}]")
        for name, t in (("length", length), ("rate_idx", rate_idx), ("n_ch", n_ch)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B, self.S):
                raise E(f"WaveStage: {name} must be int32 [B, {self.S}]")
        if select is not None:
            if self.segments < 2:
                raise E("WaveStage: select= needs segments > 1")
            if not isinstance(select, torch.Tensor) or select.dtype != torch.int32 or tuple(select.shape) != (B,):
                raise E("WaveStage: select must be int32 [B]")
        for name, t in (("raw", raw), ("length", length), ("rate_idx", rate_idx), ("n_ch", n_ch), ("select", select)):
            if t is None:
                continue
            if not t.is_cuda:
                raise E(f"WaveStage: {name} is a CPU tensor; the wave stage needs HIP device tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise E(f"WaveStage: {name} must be contiguous")
        return B

    def __call__(self, raw: torch.Tensor, length: torch.Tensor, rate_idx: torch.Tensor, n_ch: torch.Tensor,
                 select: Optional[torch.Tensor] = None, out: Optional[WaveResult] = None) -> WaveResult:
        """out: a previous result of the same shape whose buffer is written again (a static address for a captured graph)."""
        B = self._check_inputs(raw, length, rate_idx, n_ch, select)
        state = self._ensure()
        dev = self.device
        for t in (raw, length, rate_idx, n_ch, select):
            if t is not None and t.device != dev:
                raise _lib.CavpError(f"WaveStage lives on {dev}, an input on {t.device}")
        A_out = self.out_len(select is not None)
        if out is None:
            out = WaveResult(B, A_out, dev)
        else:
            w = out.waveform
            if tuple(w.shape) != (B, 1, A_out) or w.dtype != torch.float32 or w.device != dev or not w.is_contiguous():
                raise _lib.CavpError("WaveStage: out= was made for other shapes")
        lib = _lib.load()
        _lib.check(lib.cavp_wave_stage(_ptr(raw), 1 if raw.dtype == torch.int16 else 0, _ptr(length), _ptr(rate_idx), _ptr(n_ch),
                                       _ptr(select), B, self.S, self.C, self.Lmax, self.sample_len, self.segments, _ptr(self._desc),
                                       len(self.rates), _ptr(self._taps), _ptr(self._first), self.tab_cap, self.first_cap, self.x_cap,
                                       _ptr(state), _ptr(out.waveform), C.c_void_p(_stream())), "cavp_wave_stage")
        return out
