"""The device wave stage (cavp_amd/wave.py, csrc/wave.hip).  The identity-rate path is compared for equality with
tests/golden/wave_crop.npz, written by the reference's own crop_audio (tools/make_golden_wave.py); the resampled path with the
float64 whole-clip restatement tests/_wave_ref.py under the standard float32 dot-product bound
|dev - ref64| <= (span_max + S * C + 3) * 2^-24 * M, M the same sum over |x| and |h| in float64.  The output tile is 1024:
sample_len 400 is no multiple of it, 2500 spans three tiles, 16000 sixteen; at 4800 and 16000 a short clip repeats with a period above
one tile, so that a tile is computed in two passes."""
import os

import numpy as np
import pytest
import torch

from tests import _wave_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "wave_crop.npz")
MIXED_RATES = (8000, 11025, 44100, 48000)


def _stage(**kw):
    from cavp_amd.wave import WaveStage
    kw.setdefault("max_batch", 8)
    return WaveStage(device=DEV, **kw)


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _run(ws, raw, length, rate_idx, n_ch, select=None, out=None):
    ins = _dev(raw, length, rate_idx, n_ch, select)
    keep = [None if t is None else t.clone() for t in ins]
    res = ws(*ins, out=out)
    torch.cuda.synchronize()
    for t, k in zip(ins, keep):
        assert t is None or torch.equal(t.view(torch.uint8), k.view(torch.uint8)), "an input was modified"
    assert res.waveform.dtype == torch.float32 and res.waveform.shape == (raw.shape[0], 1, ws.out_len(select is not None))
    return res.waveform.cpu().numpy()


# ---- exact on the identity-rate path ---------------------------------------------------------------------------------------------
def _golden_batch(cases, kind, dtype):
    """All fixture cases of one kind as one batch: raw [B, S, C, Lmax], NaN (float32) resp. a large value (int16) beyond each
    length, so that a read past a clip's end shows."""
    rows = [(name, sources, img_id) for name, (k, sources, img_id) in cases.items() if k == kind]
    S = len(rows[0][1])
    C = max(c for _, sources, _ in rows for _, c, _ in sources)
    Lmax = max(L for _, sources, _ in rows for _, _, L in sources)
    raw = np.full((len(rows), S, C, Lmax), 32767, dtype=np.int16)
    for b, (_, sources, _) in enumerate(rows):
        for s, (seed, c, L) in enumerate(sources):
            raw[b, s, :c, :L] = R.golden_input(seed, c, L)
    if dtype == "float32":
        f = raw.astype(np.float32) / np.float32(32768.0)
        f[raw == 32767] = np.nan
        raw = f
    length = np.array([[L for _, _, L in sources] for _, sources, _ in rows], dtype=np.int32)
    n_ch = np.array([[c for _, c, _ in sources] for _, sources, _ in rows], dtype=np.int32)
    select = np.array([img_id - 1 for _, _, img_id in rows], dtype=np.int32) if rows[0][2] is not None else None
    return [name for name, _, _ in rows], raw, length, n_ch, select, (S, C, Lmax)


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("sample_len", R.GOLDEN_SAMPLE_LENS)
def test_identity_rate_equals_reference_fixture(sample_len, dtype):
    """Rate 16000 against the reference's crop_audio + mean / sum / view()[:, k]: clip lengths in every crop regime (1, below
    sample_len / 3, negative-start wrap, equal, longer), C = 2 mean, S = 2 sum, segments = 10 with select.  Exact."""
    gold = np.load(GOLDEN)
    cases = R.golden_cases(sample_len)
    seen = 0
    for kind in ("avss", "vpo", "avsb"):
        names, raw, length, n_ch, select, (S, C, Lmax) = _golden_batch(cases, kind, dtype)
        ws = _stage(audio_len=R.GOLDEN_AUDIO_LEN[sample_len], rates=(44100, 16000), max_sources=S, max_channels=C, max_len=Lmax,
                    segments=R.GOLDEN_SEGMENTS if select is not None else 1)
        assert ws.sample_len == sample_len
        got = _run(ws, raw, length, np.ones_like(length), n_ch, select)
        ws.check()
        for b, name in enumerate(names):
            assert np.array_equal(got[b], gold[name]), name
            seen += 1
    assert seen == len(cases) == 11


# ---- resampled path against the float64 restatement -------------------------------------------------------------------------------
def _len_for(rate, L16):
    """The shortest L with ceil(n L / o) >= L16 (equal whenever some L resamples to exactly L16 samples)."""
    L = max((L16 * rate) // 16000, 1)
    while R.target_len(L, rate) < L16:
        L += 1
    while L > 1 and R.target_len(L - 1, rate) >= L16:
        L -= 1
    return L


def _mixed_batch(sample_len, variant, rng, pad=np.float32(0.0)):
    """B = 3, S = 2, C = 2, the four rates mixed inside the batch; per source (rate index, resampled length, channels): every
    crop regime, L = 1 and an absent source over the two variants."""
    sl = sample_len
    plan = {"a": [[(0, sl, 2), (2, 2 * sl + 7, 1)], [(1, sl // 4, 2), (3, (2 * sl) // 3 + 5, 2)], [(2, (3 * sl) // 4, 1), (1, sl + sl // 2 + 1, 2)]],
            "b": [[(3, sl, 1), (0, (2 * sl) // 5 + 2, 2)], [(1, None, 2), (2, sl, 1)], [(0, 0, 1), (3, 3 * sl, 2)]]}[variant]
    length = np.zeros((3, 2), np.int32)
    rate_idx = np.zeros((3, 2), np.int32)
    n_ch = np.ones((3, 2), np.int32)
    for b in range(3):
        for s in range(2):
            r, L16, c = plan[b][s]
            rate_idx[b, s], n_ch[b, s] = r, c
            length[b, s] = 1 if L16 is None else 0 if L16 == 0 else _len_for(MIXED_RATES[r], L16)
    Lmax = int(length.max()) + 3
    raw = rng.uniform(-1, 1, (3, 2, 2, Lmax)).astype(np.float32)
    if pad is not None:
        for b in range(3):
            for s in range(2):
                raw[b, s, :, length[b, s]:] = pad
                raw[b, s, n_ch[b, s]:] = pad
    return raw, length, rate_idx, n_ch, Lmax


def _assert_within_bound(ws, got, raw, length, rate_idx, n_ch, sample_len, segments=1, select=None):
    want, bad = R.wave_ref(raw, length, rate_idx, n_ch, ws.rates, sample_len, segments, select)
    M, _ = R.wave_ref(raw, length, rate_idx, n_ch, ws.rates, sample_len, segments, select, absolute=True)
    assert bad == 0
    B, S, C, _ = raw.shape
    span_max = max(tb["span"] for tb in ws.tables)
    tol = (span_max + S * C + 3) * 2.0 ** -24 * M
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"sample_len {sample_len}: max |dev - ref64| {err.max():.3e}, largest share of the bound {worst:.3f}")
    assert np.all(err <= tol)
    assert np.abs(want).max() > 0.1


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("sample_len", [400, 2500, 4800])
def test_resampled_mixed_rates_within_f32_bound(sample_len, variant):
    rng = np.random.default_rng(sample_len + ord(variant))
    raw, length, rate_idx, n_ch, Lmax = _mixed_batch(sample_len, variant, rng)
    ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=MIXED_RATES, max_sources=2, max_channels=2, max_len=Lmax)
    assert ws.sample_len == sample_len
    got = _run(ws, raw, length, rate_idx, n_ch)
    ws.check()
    _assert_within_bound(ws, got, raw, length, rate_idx, n_ch, sample_len)
    L16 = [R.target_len(length[b, s], MIXED_RATES[rate_idx[b, s]]) for b in range(3) for s in range(2)]
    assert sample_len in L16 and max(L16) > sample_len and 0 < min(v for v in L16 if v) < sample_len / 3
    if variant == "b":
        assert length[2, 0] == 0 and length[1, 0] == 1


def test_select_on_resampled_clips():
    sample_len, segments = 2500, 10
    rng = np.random.default_rng(5)
    raw, length, rate_idx, n_ch, Lmax = _mixed_batch(sample_len, "a", rng)
    select = np.array([9, 0, 4], dtype=np.int32)
    ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=MIXED_RATES, max_sources=2, max_channels=2, max_len=Lmax, segments=segments)
    got = _run(ws, raw, length, rate_idx, n_ch, select)
    whole = _run(ws, raw, length, rate_idx, n_ch)
    ws.check()
    _assert_within_bound(ws, got, raw, length, rate_idx, n_ch, sample_len, segments, select)
    for b in range(3):
        assert np.array_equal(got[b, 0], whole[b, 0].reshape(segments, -1)[select[b]])


def test_nan_padding_is_never_read():
    """NaN beyond each source's length, in the unused channels and in the absent source: finite output, the same bits."""
    sample_len = 2500
    for variant in ("a", "b"):
        clean = _mixed_batch(sample_len, variant, np.random.default_rng(11))
        dirty = _mixed_batch(sample_len, variant, np.random.default_rng(11), pad=np.float32(np.nan))
        assert np.isnan(dirty[0]).any()
        ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=MIXED_RATES, max_sources=2, max_channels=2, max_len=clean[4])
        a = _run(ws, *clean[:4])
        b = _run(ws, *dirty[:4])
        assert np.isfinite(b).all() and np.array_equal(a, b)


@pytest.mark.parametrize("with_select", [False, True])
def test_output_stays_inside_its_buffer(with_select):
    from cavp_amd.wave import WaveResult
    sample_len, segments, G = 2500, 10, 4096
    raw, length, rate_idx, n_ch, Lmax = _mixed_batch(sample_len, "a", np.random.default_rng(3))
    ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=MIXED_RATES, max_sources=2, max_channels=2, max_len=Lmax, segments=segments)
    A_out = ws.out_len(with_select)
    buf = torch.full((G + 3 * A_out + G,), -77.0, dtype=torch.float32, device=DEV)
    res = WaveResult(3, 1, DEV)
    res.waveform = buf[G:G + 3 * A_out].view(3, 1, A_out)
    select = np.array([9, 0, 4], dtype=np.int32) if with_select else None
    got = _run(ws, raw, length, rate_idx, n_ch, select, out=res)
    host = buf.cpu().numpy()
    assert np.all(host[:G] == -77.0) and np.all(host[-G:] == -77.0)
    assert np.array_equal(host[G:-G].reshape(3, 1, A_out), got) and not np.any(got == -77.0)
    fresh = _run(ws, raw, length, rate_idx, n_ch, select)
    assert np.array_equal(fresh, got)


def test_index_math_is_64_bit():
    """One source of 3 355 500 samples at 11025 Hz: n * L = 640 * L > 2^31."""
    rate, L, sample_len = 11025, 3355500, 400
    assert 640 * L > 2 ** 31
    rng = np.random.default_rng(7)
    raw = rng.uniform(-1, 1, (1, 1, 1, L)).astype(np.float32)
    length, rate_idx, n_ch = (np.array([[v]], dtype=np.int32) for v in (L, 1, 1))
    ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=(16000, rate), max_sources=1, max_channels=1, max_len=L)
    got = _run(ws, raw, length, rate_idx, n_ch)
    ws.check()
    _assert_within_bound(ws, got, raw, length, rate_idx, n_ch, sample_len)


def test_bad_inputs_are_counted_and_zeroed():
    from cavp_amd._lib import CavpError
    sample_len, segments, Lmax, B = 400, 10, 700, 7
    rng = np.random.default_rng(13)
    raw = rng.uniform(-1, 1, (B, 2, 2, Lmax)).astype(np.float32)
    length = np.full((B, 2), 600, np.int32)
    rate_idx = np.zeros((B, 2), np.int32)
    n_ch = np.full((B, 2), 2, np.int32)
    select = np.arange(B, dtype=np.int32)
    length[1, 1] = Lmax + 1                 # bad
    length[2, 0] = -1                       # bad
    rate_idx[3, 1] = 2                      # bad: two rates
    n_ch[4, 0] = 3                          # bad: C = 2
    n_ch[4, 1] = 0                          # bad
    length[5, 0], rate_idx[5, 0], n_ch[5, 0] = 0, 99, 99      # an absent source: its rate_idx and n_ch are not looked at
    select[6] = segments                    # bad
    ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=(16000, 8000), max_sources=2, max_channels=2, max_len=Lmax, segments=segments)
    want, bad = R.wave_ref(raw, length, rate_idx, n_ch, ws.rates, sample_len, segments, select)
    assert bad == 6
    got = _run(ws, raw, length, rate_idx, n_ch, select)
    for b in (1, 2, 3, 4, 6):
        assert not got[b].any()
    for b in (0, 5):
        assert got[b].any() and np.abs(got[b] - want[b]).max() <= 4 * 2.0 ** -24 * 2      # identity rate: two means, one add
    with pytest.raises(CavpError, match="6 input value"):
        ws.check()
    ws.check()                              # the counter was cleared by the report
    # without select the same rows are bad but the last
    got = _run(ws, raw, length, rate_idx, n_ch)
    assert got[6].any() and not got[4].any()
    with pytest.raises(CavpError, match="5 input value"):
        ws.check()


def test_two_calls_are_bit_identical():
    sample_len = 2500
    raw, length, rate_idx, n_ch, Lmax = _mixed_batch(sample_len, "a", np.random.default_rng(17))
    ws = _stage(audio_len=sample_len / 16000 + 1e-9, rates=MIXED_RATES, max_sources=2, max_channels=2, max_len=Lmax)
    a = _run(ws, raw, length, rate_idx, n_ch)
    b = _run(ws, raw, length, rate_idx, n_ch)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_graph_capture_with_pair_builder_and_mel_frontend():
    """WaveStage -> PairBuilder -> MelFrontEnd captured in one graph on out= buffers (capture raises if anything synchronises or
    allocates on the host's behalf); after the staging buffers are rewritten, a replay equals eager calls on the new data."""
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.pairs import PairBuilder
    B, K, A, hw, Lmax, seed = 4, 6, 16000, 8, 50000, 21
    rng = np.random.default_rng(seed)

    def batch():
        raw = rng.integers(-20000, 20000, (B, 1, 2, Lmax)).astype(np.int16)
        length = rng.integers(20000, Lmax + 1, (B, 1)).astype(np.int32)
        return raw, length

    rate_idx = torch.zeros((B, 1), dtype=torch.int32, device=DEV)
    n_ch = torch.full((B, 1), 2, dtype=torch.int32, device=DEV)
    img = np.zeros((B, K), np.int64)
    img[np.arange(B), 1 + np.arange(B) % 3] = 1
    pix_label, img_label = _dev(rng.integers(0, K, (B, hw, hw)).astype(np.int64), img)
    raw, length = _dev(*batch())

    def make():
        return (_stage(audio_len=1.0, rates=(44100, 16000), max_sources=1, max_channels=2, max_len=Lmax),
                PairBuilder(num_classes=K, bank_slots=2, wave_len=A, ow_rate=0.5, seed=seed, device=DEV, max_batch=8))

    (ws, pb), (ws_e, pb_e) = make(), make()
    mel = MelFrontEnd(None, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w_out = ws(raw, length, rate_idx, n_ch)
        p_out = pb(w_out.waveform, pix_label, img_label, True)
        mel(p_out.waveforms)
    torch.cuda.current_stream().wait_stream(side)
    pb_e(ws_e(raw, length, rate_idx, n_ch).waveform, pix_label, img_label, True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ws(raw, length, rate_idx, n_ch, out=w_out)
        pb(w_out.waveform, pix_label, img_label, True, out=p_out)
        spec = mel(p_out.waveforms)
    for _ in range(2):
        new_raw, new_length = _dev(*batch())
        raw.copy_(new_raw)
        length.copy_(new_length)
        graph.replay()
        torch.cuda.synchronize()
        w_e = ws_e(new_raw, new_length, rate_idx, n_ch)
        p_e = pb_e(w_e.waveform, pix_label, img_label, True)
        assert torch.equal(w_out.waveform, w_e.waveform) and w_e.waveform.abs().max() > 0.01
        assert torch.equal(p_out.waveforms, p_e.waveforms) and torch.equal(p_out.label_shuffle, p_e.label_shuffle)
        assert torch.equal(spec, mel(p_e.waveforms))
    ws.check()


def test_non_contiguous_and_misshapen_device_inputs_raise():
    from cavp_amd._lib import CavpError
    from cavp_amd.wave import WaveResult
    ws = _stage(audio_len=0.025, rates=(16000,), max_sources=2, max_channels=2, max_len=100)
    raw = torch.zeros((3, 2, 2, 200), device=DEV)
    i32 = torch.ones((3, 2), dtype=torch.int32, device=DEV)
    wide = torch.ones((3, 4), dtype=torch.int32, device=DEV)
    r0 = torch.zeros((3, 2), dtype=torch.int32, device=DEV)
    with pytest.raises(CavpError, match="contiguous"):
        ws(raw[:, :, :, ::2], i32, r0, i32)
    with pytest.raises(CavpError, match="contiguous"):
        ws(raw[:, :, :, :100].contiguous(), wide[:, ::2], r0, i32)
    with pytest.raises(CavpError):
        ws(raw[:, :, :, :100].contiguous(), i32, r0, i32, out=WaveResult(3, 399, DEV))
    ok = ws(raw[:, :, :, :100].contiguous(), i32, r0, i32)
    assert ok.waveform.shape == (3, 1, 400) and not ok.waveform.any()
    ws.check()
