"""The device pair builder (cavp_amd/pairs.py, csrc/pairs.hip) against the reference's recorded steps (tests/golden/pairs.npz) and
against the numpy restatement of its specification (tests/_pairs_ref.py).  Everything it produces is a copy or an integer:
every comparison is exact equality."""
import numpy as np
import pytest
import torch

from tests import _pairs_ref as R
from tests.test_pairs_host import _replay, assert_step_equals_golden, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("waveforms", "label_shuffle", "if_match", "img_label_shuffle", "perm", "source")


def _builder(K, S, A, rate=0.5, seed=0, max_batch=64):
    from cavp_amd.pairs import PairBuilder
    return PairBuilder(num_classes=K, bank_slots=S, wave_len=A, ow_rate=rate, seed=seed, device=DEV, max_batch=max_batch)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _host(out):
    return {f: getattr(out, f).cpu().numpy() for f in FIELDS}


def _batch(rng, B, K, A, hw, step):
    """Rows mix single-source, two-source and background-only image labels; from B = 5 on, step 2 has five rows of class 1 in one
    batch (more pushes to one class than a bank of 2 slots holds)."""
    img = np.zeros((B, K), dtype=np.int64)
    for i in range(B):
        kind = rng.random()
        img[i, 0] = rng.integers(0, 2)
        if kind < 0.6 or K == 2 and kind < 0.8:
            img[i, rng.integers(1, min(K, 4))] = 1
        elif kind < 0.8:
            img[i, rng.choice(np.arange(1, K), size=2, replace=False)] = 1
        else:
            img[i, 0] = 1
    if step == 2 and B >= 5:
        img[:5] = 0
        img[:5, 1] = 1
    wav = rng.standard_normal((B, 1, A)).astype(np.float32)
    pix = rng.integers(0, K, (B, hw, hw)).astype(np.int64)
    return wav, pix, img


def _assert_equals_ref(out, pb, exp, ref):
    got = _host(out)
    for f in FIELDS:
        assert np.array_equal(got[f], exp[f]), f
    assert np.array_equal(pb.bank_vault.cpu().numpy(), ref.bank)


def test_fixture_replay():
    """The reference's 8 recorded steps with its own torch.randperm draws fed in: every output and the bank after every step."""
    g = golden()
    B, K, S, A, H, W, steps = (int(v) for v in g["config"])
    pb = _builder(K, S, A, float(g["ow_rate"]), max_batch=B)
    for s in range(steps):
        wav, pix, img, perm = _dev(g["waveform"][s], g["pix_label"][s], g["img_label"][s], g["perm"][s])
        ow = bool(g["overwrite"][s])
        rank = _dev(R.rank_from_draw(g["if_match_shuffle"][s], g["ow_draw"][s]))[0] if ow else None
        out = pb(wav, pix, img, ow, perm=perm, ow_rank=rank)
        assert_step_equals_golden(_host(out), pb.bank_vault.cpu().numpy(), g, s)
        plan = pb.last_plan()
        assert plan["n_false"] == int(g["n_false"][s]) and plan["n_overwritten"] == int((g["mod_idx_map"][s] >= 0).sum())


@pytest.mark.parametrize("hw", [7, 8])
@pytest.mark.parametrize("S,A", [(2, 62), (4, 64), (33, 16000)])
@pytest.mark.parametrize("K", [2, 6, 24])
@pytest.mark.parametrize("B", [1, 2, 8, 33])
def test_restatement_grid(B, K, S, A, hw):
    """The builder's own Philox draws: six chained steps equal the restatement index for index (A = 62 and hw = 7 take the 4-byte
    and 8-byte paths, B = 33 pads the sort to 64, S = 2 meets five pushes to one class in one batch, B = 1 has n_false = 0)."""
    seed = 1000 * B + 10 * K + S
    rng = np.random.default_rng(seed)
    pb, ref = _builder(K, S, A, seed=seed), R.PairsRef(K, S, A, 0.5, seed=seed)
    overwritten = 0
    for step in range(6):
        wav, pix, img = _batch(rng, B, K, A, hw, step)
        exp = ref(wav, pix, img, step >= 1)
        out = pb(*_dev(wav, pix, img), step >= 1)
        _assert_equals_ref(out, pb, exp, ref)
        plan = pb.last_plan()
        assert (plan["n_false"], plan["q"], plan["offset"], plan["seed"]) == (exp["n_false"], exp["q"], step, seed)
        overwritten += plan["n_overwritten"]
        if S == 2 and B >= 5 and step == 2:
            assert plan["n_written"] <= 2 * (K - 1) and (plan["wr_table"][:3] == -1).all()      # rows 0..2 of class 1 are pushed out again
    if B == 1:
        assert overwritten == 0
    if B >= 8 and K <= 6:
        assert overwritten > 0


def test_limit_batch_1024():
    B, K, S, A, hw, seed = 1024, 6, 4, 8, 2, 5
    rng = np.random.default_rng(seed)
    pb, ref = _builder(K, S, A, seed=seed, max_batch=1024), R.PairsRef(K, S, A, 0.5, seed=seed)
    for step in range(2):
        wav, pix, img = _batch(rng, B, K, A, hw, step)
        exp = ref(wav, pix, img, True)
        _assert_equals_ref(pb(*_dev(wav, pix, img), True), pb, exp, ref)
    assert pb.last_plan()["n_overwritten"] > 0


def test_ordering_hazard():
    """Row 0 is overwritten from class 1 while rows 0 and 2 push to class 1, whose two slots are both replaced in this step: the
    overwritten clip must be the OLD slot 0 bit for bit (the gather launch precedes the bank update)."""
    K, S, A, hw = 3, 2, 16000, 8
    g = torch.Generator().manual_seed(3)
    pb = _builder(K, S, A, rate=0.5)
    loaded = torch.randn((K, S, A), generator=g)
    pb.load_bank(loaded.to(DEV))
    img0 = torch.tensor([[0, 1, 0], [0, 0, 0], [1, 0, 0]], dtype=torch.int64)
    wav0 = torch.randn((3, 1, A), generator=g)
    pix = torch.randint(0, K, (3, hw, hw), generator=g)
    ident = torch.arange(3, dtype=torch.int32)
    pb(wav0.to(DEV), pix.to(DEV), img0.to(DEV), False, perm=ident.to(DEV))          # one push to class 1: its ring head is at 1 now
    old = pb.bank_vault.cpu()
    assert torch.equal(old[1], torch.stack([loaded[1, 1], wav0[0, 0]])) and int(pb.last_plan()["head"][1]) == 1
    img = torch.tensor([[0, 1, 0], [0, 0, 1], [0, 1, 0]], dtype=torch.int64)
    wav = torch.randn((3, 1, A), generator=g)
    perm = torch.tensor([1, 0, 2], dtype=torch.int32)          # rows 0 and 1 mismatch: n_false = 2, q = 1
    rank = torch.tensor([0, 1, 2], dtype=torch.int32)          # row 0 is the pick
    out = pb(wav.to(DEV), pix.to(DEV), img.to(DEV), True, perm=perm.to(DEV), ow_rank=rank.to(DEV))
    plan = pb.last_plan()
    assert (plan["n_false"], plan["q"], plan["n_overwritten"], plan["n_written"]) == (2, 1, 1, 3)
    assert out.source.cpu().tolist() == [~1, 0, 2] and out.if_match.cpu().tolist() == [1, 0, 1]
    assert torch.equal(out.waveforms[3].cpu(), old[1, 0][None])
    assert torch.equal(out.waveforms[4:].cpu(), wav[[0, 2]])
    new = pb.bank_vault.cpu()
    assert torch.equal(new[1], torch.stack([wav[0, 0], wav[2, 0]])) and torch.equal(new[2], torch.stack([old[2, 1], wav[1, 0]]))


def test_inputs_are_not_modified_and_bad_labels_are_reported():
    from cavp_amd._lib import CavpError
    B, K, S, A, hw = 8, 6, 4, 64, 8
    rng = np.random.default_rng(11)
    pb = _builder(K, S, A)
    for step in range(2):
        ins = _dev(*_batch(rng, B, K, A, hw, step))
        kept = [t.clone() for t in ins]
        pb(*ins, True)
        assert all(torch.equal(a, b) for a, b in zip(ins, kept))
    pb.last_plan()
    ins[2][3, 2] = 2
    pb(*ins, True)
    with pytest.raises(CavpError, match="out of range"):
        pb.last_plan()
    pb.last_plan()          # the counter was cleared by the report


def test_graph_capture_with_mel_frontend():
    """Builder + MelFrontEnd as one captured graph on out= buffers (capture raises if anything synchronises): three replays draw
    three different permutations and advance the bank exactly as three eager calls from the same seed and state do."""
    from cavp_amd.audio_frontend import MelFrontEnd
    B, K, S, A, hw, seed = 8, 6, 2, 16000, 8, 9
    rng = np.random.default_rng(seed)
    ins = _dev(*_batch(rng, B, K, A, hw, 0))
    mel = MelFrontEnd(None, device=DEV)
    pb, eager = _builder(K, S, A, seed=seed), _builder(K, S, A, seed=seed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = pb(*ins, True)
        mel(out.waveforms)
    torch.cuda.current_stream().wait_stream(side)
    eager(*ins, True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pb(*ins, True, out=out)
        spec = mel(out.waveforms)
    perms = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got, bank, spec_g = _host(out), pb.bank_vault.clone(), spec.clone()
        e = eager(*ins, True)
        exp = _host(e)
        for f in FIELDS:
            assert np.array_equal(got[f], exp[f]), (k, f)
        assert torch.equal(bank, eager.bank_vault) and torch.equal(spec_g, mel(e.waveforms))
        assert pb.last_plan()["offset"] == 1 + k
        assert np.array_equal(got["perm"], R.draw_perm(B, seed, 1 + k))
        perms.append(got["perm"].tolist())
    assert perms[0] != perms[1] != perms[2] != perms[0]


def test_train_step_on_builder_outputs(deterministic):
    """B = 4, 64 x 64, bf16, fixed-order reductions, host anchor sampler under one torch seed: the native CE + contrast step fed the
    builder's outputs equals the step fed the restatement's outputs - the loss and every gradient bit for bit."""
    from cavp_amd.audio_frontend import MelFrontEnd
    from cavp_amd.contrast import ContrastLoss
    from cavp_amd.synth import synth_inputs
    from tests.test_gpu_train_model import _build
    cfg = dict(C=3, B=4, hw=(64, 64), lds=[False, False, False])
    B, K, S, A, seed = 4, 3, 2, 16000, 2
    image, _, label = synth_inputs(B, cfg["hw"], audio_batch=2 * B, num_classes=K, seed=21)
    label[:, 8:40, 8:48] = 1
    label[:, 44:60, 4:60] = 2
    rng = np.random.default_rng(seed)
    pb, ref = _builder(K, S, A, rate=1.0, seed=seed), R.PairsRef(K, S, A, 1.0, seed=seed)
    img = np.array([[0, 1, 0], [0, 0, 1], [0, 1, 0], [1, 1, 1]], dtype=np.int64)
    for step in range(3):
        wav = rng.standard_normal((B, 1, A)).astype(np.float32)
        exp = ref(wav, label.numpy(), img, step >= 1)
        out = pb(*_dev(wav, label.numpy(), img), step >= 1)
    mel = MelFrontEnd(None, device=DEV)
    results = []
    for waves, shuf in ((out.waveforms, out.label_shuffle), tuple(_dev(exp["waveforms"], exp["label_shuffle"]))):
        m, _ = _build(cfg, torch.bfloat16)
        torch.manual_seed(77)
        loss = m.train_step(image.to(DEV), mel(waves), label.to(DEV), contrast=ContrastLoss(0.1, 255, 32), label_shuffle=shuf)
        torch.cuda.synchronize()
        results.append((loss.clone(), [t.clone() for t in m._last_losses], m))
    (l1, t1, m1), (l2, t2, m2) = results
    assert float(t1[1].item()) > 0.0
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(t1, t2))
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), k
        if p1.grad is not None:
            assert torch.equal(p1.grad, p2.grad), k
