"""Wave stage, host side (no GPU): the exported symbols, the float64 restatement tests/_wave_ref.py against the fixture written by
the reference's own crop_audio, the resampler against an analytic tone, the compact filter table of cavp_amd/wave.py against the
full table, and the constructor's and the call's host checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _wave_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "wave_crop.npz")
RATES = (8000, 11025, 22050, 32000, 44100, 48000)
SPANS = {8000: 13, 11025: 13, 22050: 17, 32000: 25, 44100: 34, 48000: 37}


def test_library_exports_wave_stage():
    from cavp_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cavp_wave_stage", "cavp_wave_tile"):
        assert hasattr(lib, name), f"libcavp_hip.so does not export {name}"
        assert name in _lib.PROTOTYPES
    bound = _lib.load()
    assert _lib.ABI_VERSION == bound.cavp_abi_version() == 16
    from cavp_amd import wave
    assert bound.cavp_wave_tile() == wave.TILE


def _golden_ref(name, kind, sources, img_id, sample_len, as_int16):
    """The restatement on one fixture case: (out, expected)."""
    S, C = len(sources), max(c for _, c, _ in sources)
    Lmax = max(L for _, _, L in sources)
    raw = np.zeros((1, S, C, Lmax), dtype=np.int16)
    for s, (seed, c, L) in enumerate(sources):
        raw[0, s, :c, :L] = R.golden_input(seed, c, L)
    length = np.array([[L for _, _, L in sources]], dtype=np.int32)
    n_ch = np.array([[c for _, c, _ in sources]], dtype=np.int32)
    rate_idx = np.zeros((1, S), dtype=np.int32)
    select = np.array([img_id - 1], dtype=np.int32) if img_id is not None else None
    x = raw if as_int16 else raw.astype(np.float32) / np.float32(32768.0)
    out, bad = R.wave_ref(x, length, rate_idx, n_ch, (16000,), sample_len, R.GOLDEN_SEGMENTS if select is not None else 1, select)
    assert bad == 0
    return out[0]


@pytest.mark.parametrize("sample_len", R.GOLDEN_SAMPLE_LENS)
def test_restatement_reproduces_reference_crop(sample_len):
    gold = np.load(GOLDEN)
    cases = R.golden_cases(sample_len)
    assert len(cases) == 11
    for name, (kind, sources, img_id) in cases.items():
        for as_int16 in (False, True):
            out = _golden_ref(name, kind, sources, img_id, sample_len, as_int16)
            assert out.shape == gold[name].shape, name
            assert np.array_equal(out, gold[name].astype(np.float64)), name


def test_crop_rule_equals_reference_expression():
    for sample_len in (64, 65, 400):
        for L16 in list(range(1, 400)) + [sample_len * 3, sample_len * 3 + 1]:
            y = torch.arange(2 * L16, dtype=torch.float64).reshape(2, L16)
            s0, ln = R.crop_range(L16, sample_len)
            assert ln >= 1
            assert np.array_equal(R.crop(y.numpy(), sample_len), R.crop_audio_literal(y, sample_len).numpy()), (sample_len, L16)


def test_restatement_identity_rate():
    x = np.random.default_rng(0).uniform(-1, 1, (2, 777))
    assert np.array_equal(R.resample64(x, 16000), x)
    assert R.target_len(777, 16000) == 777


@pytest.mark.parametrize("rate", RATES)
def test_restatement_resamples_a_tone(rate):
    """A 2 s unit tone at 440 Hz: interior (200 samples off each end) error against the analytic 16 kHz tone at most 1e-3; a wrong
    phase sign or width shifts the signal by at least one source sample, an error of at least 0.06."""
    L = 2 * rate
    x = np.sin(2 * np.pi * 440.0 * np.arange(L) / rate)
    y = R.resample64(x[None], rate)[0]
    assert y.shape[0] == R.target_len(L, rate) == 32000
    want = np.sin(2 * np.pi * 440.0 * np.arange(y.shape[0]) / 16000.0)
    err = np.abs(y - want)[200:-200].max()
    print(f"rate {rate}: interior error {err:.3e}")
    assert err <= 1e-3


@pytest.mark.parametrize("rate", RATES)
def test_compact_table_is_the_full_table(rate):
    """Everything outside [first, first + span) of each phase of the full float32 table is exactly 0.0f, the compact rows hold the
    rest bit for bit, and the spans are the documented ones."""
    from cavp_amd import wave
    h, o, n, width = R.full_kernel(rate)
    tb = wave.compact_table(rate)
    assert (tb["o"], tb["n"], tb["width"], tb["span"]) == (o, n, width, SPANS[rate])
    assert tb["stride"] % 2 == 1 and tb["stride"] >= tb["span"] and tb["taps"].nbytes <= 33280
    fmin = tb["shift"] + width
    assert tb["first"].min() == 0 and tb["first"].max() == tb["fspread"]
    for p in range(n):
        f = fmin + int(tb["first"][p])
        full = np.zeros(h.shape[1] + tb["stride"], np.float32)
        full[f:f + tb["stride"]] = tb["taps"][p]
        assert np.array_equal(full[:h.shape[1]], h[p]) and not full[h.shape[1]:].any(), (rate, p)


def _window_only(ws, raw, length, rate_idx, n_ch, select=None):
    """The device's evaluation order in float64 on the host: compact table, only the cropped window of y (rules 1-4)."""
    B, S, C, Lmax = raw.shape
    A_out = ws.out_len(select is not None)
    out = np.zeros((B, 1, A_out))
    x_all = raw.astype(np.float64) / 32768.0 if raw.dtype == np.int16 else raw.astype(np.float64)
    for b in range(B):
        woff = int(select[b]) * A_out if select is not None else 0
        for s in range(S):
            L = int(length[b, s])
            if L == 0:
                continue
            o, n, span, stride, tap_off, first_off, shift, _ = (int(v) for v in ws.desc_host[int(rate_idx[b, s])])
            taps = ws.taps_host[tap_off:tap_off + n * stride].reshape(n, stride).astype(np.float64)
            first = ws.first_host[first_off:first_off + n]
            L16 = -((-n * L) // o)
            s0, ln = R.crop_range(L16, ws.sample_len)
            i = woff + np.arange(A_out)
            j = s0 + (i if ln == ws.sample_len else i % ln)
            p, q = j % n, j // n
            idx = (q * o + shift + first[p])[:, None] + np.arange(span)[None, :]
            nc = int(n_ch[b, s])
            m = np.zeros(A_out)
            for c in range(nc):
                xz = np.where((idx >= 0) & (idx < L), x_all[b, s, c][np.clip(idx, 0, L - 1)], 0.0)
                m += (taps[p, :span] * xz).sum(1)
            out[b, 0] += m / nc
    return out


def test_window_only_evaluation_equals_whole_clip_restatement():
    from cavp_amd import wave
    rates = (16000,) + RATES
    rng = np.random.default_rng(1)
    sample_len, segments = 330, 10
    ws = wave.WaveStage(audio_len=sample_len / 16000 + 1e-9, rates=rates, max_sources=2, max_channels=2, max_len=1500, segments=segments)
    assert ws.sample_len == sample_len
    B = 8
    raw = rng.uniform(-1, 1, (B, 2, 2, 1500)).astype(np.float32)
    length = rng.integers(1, 1501, (B, 2)).astype(np.int32)
    length[0] = (1, 0)
    length[1] = (1500, 40)
    rate_idx = rng.integers(0, len(rates), (B, 2)).astype(np.int32)
    n_ch = rng.integers(1, 3, (B, 2)).astype(np.int32)
    for select in (None, rng.integers(0, segments, B).astype(np.int32)):
        want, bad = R.wave_ref(raw, length, rate_idx, n_ch, rates, sample_len, segments, select)
        assert bad == 0
        got = _window_only(ws, raw, length, rate_idx, n_ch, select)
        assert np.abs(got - want).max() <= 1e-13


def test_restatement_counts_bad_rows():
    raw = np.ones((4, 1, 1, 50), np.float32)
    length = np.array([[50], [51], [50], [50]], np.int32)
    rate_idx = np.array([[0], [0], [2], [0]], np.int32)
    n_ch = np.array([[1], [1], [1], [0]], np.int32)
    out, bad = R.wave_ref(raw, length, rate_idx, n_ch, (16000, 8000), 20)
    assert bad == 3 and out[0].all() and not out[1:].any()


def test_constructor_limits():
    from cavp_amd import wave
    from cavp_amd._lib import CavpError
    kw = dict(audio_len=1.0, max_sources=1, max_channels=2, max_len=1000)
    wave.WaveStage(rates=(16000, 4000, 192000), **kw)
    for rates in ((3999,), (192001,), (44101,), (16000.5,), (), (8000,) * 9):
        with pytest.raises(CavpError):
            wave.WaveStage(rates=rates, **kw)
    with pytest.raises(CavpError):
        wave.WaveStage(audio_len=1.0, rates=(16000,), max_sources=1, max_channels=1, max_len=1000, segments=7)      # 16000 % 7
    with pytest.raises(CavpError):
        wave.WaveStage(audio_len=0.0, rates=(16000,), max_sources=1, max_channels=1, max_len=1000)
    for bad in (dict(max_sources=0), dict(max_channels=0), dict(max_len=0), dict(max_len=(1 << 28) + 1), dict(max_batch=0)):
        with pytest.raises(CavpError):
            wave.WaveStage(**{**kw, "rates": (16000,), **bad})
    assert wave.WaveStage(audio_len=0.96, rates=(16000,), max_sources=1, max_channels=1, max_len=10).sample_len == int(0.96 * 16000)


def test_cpu_tensors_and_wrong_inputs_raise():
    from cavp_amd import wave
    from cavp_amd._lib import CavpError
    ws = wave.WaveStage(audio_len=0.025, rates=(16000, 44100), max_sources=2, max_channels=2, max_len=100, segments=10)
    raw = torch.zeros((3, 2, 2, 100))
    i32 = torch.ones((3, 2), dtype=torch.int32)
    with pytest.raises(CavpError, match="CPU tensor"):
        ws(raw, i32, i32, i32)
    with pytest.raises(CavpError):
        ws(raw.double(), i32, i32, i32)
    with pytest.raises(CavpError):
        ws(raw[:, :, :, :99], i32, i32, i32)
    with pytest.raises(CavpError):
        ws(raw, i32.long(), i32, i32)
    with pytest.raises(CavpError):
        ws(raw, i32, i32[:2], i32)
    with pytest.raises(CavpError):
        ws(raw, i32, i32, i32, select=torch.zeros(2, dtype=torch.int32))
    ws1 = wave.WaveStage(audio_len=0.025, rates=(16000,), max_sources=2, max_channels=2, max_len=100)
    with pytest.raises(CavpError, match="segments"):
        ws1(raw, i32, i32, i32, select=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(CavpError, match="no WaveStage call yet"):
        ws.check()
