"""The float64 attention references, the input families and the cases of test_gpu_attention_edges.py have teeth (CPU only):
autograd of each reference against finite differences, the explicit SRA formulas against autograd, the conditions every input
family promises, and - for every GPU case, in both dtypes - deliberately wrong float64 evaluations that must land outside the bar
the GPU test holds the kernel to."""
import pytest
import torch

from tests import _attn_ref as R

F32, BF = torch.float32, torch.bfloat16
DT = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])


def _rand(*shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_gradcheck_of_the_references():
    q, kv = _rand(1, 3, 8, seed=1).requires_grad_(True), _rand(1, 5, 16, seed=2).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: R.sra_ref(a, b, 2, 0.5), (q, kv))
    q, k, v = (_rand(*s, seed=3 + i).requires_grad_(True) for i, s in enumerate(((2, 3, 8), (4, 8), (4, 8))))
    assert torch.autograd.gradcheck(lambda a, b, c: R.gate_ref(a, b, c, 2, 0.5, 2), (q, k, v))
    x, k, v, wq, wp, bp = (_rand(*s, seed=6 + i).requires_grad_(True) for i, s in enumerate(((2, 3, 8), (4, 8), (4, 8), (8, 8), (8, 8), (8,))))
    assert torch.autograd.gradcheck(lambda *a: R.rank1_ref(*a, 4, 2 ** -0.5, 2), (x, k, v, wq, wp, bp))
    assert torch.autograd.gradcheck(lambda *a: R.rank1_ref(*a, None, 4, 2 ** -0.5, 2), (x, k, v, wq, wp))


@pytest.mark.parametrize("B,heads,Nq,Nk", [(2, 2, 5, 1), (1, 3, 17, 33), (2, 1, 70, 65)])
def test_explicit_sra_formulas_are_the_autograd_of_the_reference(B, heads, Nq, Nk):
    q, kv, dout = R.sra_inputs("gaussian", B, heads, Nq, Nk, seed=11)
    a, b = R.sra_grads_autograd(q, kv, dout, heads, 0.125), R.sra_eval(q, kv, dout, heads, 0.125)
    for name in a:
        assert R.rel_err(b[name], a[name]) <= 1e-13, name


def test_gate_expansion_and_per_item_dq():
    """q_batch < B: item b reads q[b % q_batch]; dq is per batch item (the sum over the items is the caller's)."""
    q, k, v, dout, dattn = R.gate_inputs("gaussian", 2, 4, 3, 4, 2, True, seed=12)
    r = R.gate_eval(q, k, v, dout, dattn, 2, 0.5)
    for b in range(4):
        one = R.gate_eval(q[b % 2:b % 2 + 1], k[b:b + 1], v[b:b + 1], dout[b:b + 1], dattn[b:b + 1], 2, 0.5)
        for name in r:
            assert torch.equal(one[name][0], r[name][b]), (b, name)


def test_rank1_dx_sums_the_repeats():
    x, k, v, wq, wp, bp, dout = R.rank1_inputs("gaussian", 16, 3, 2, 3, True, seed=13)
    r = R.rank1_eval(x, k, v, wq, wp, bp, dout, 4, 0.5, 3)
    xr = x.double().requires_grad_(True)
    out, _ = R.rank1_ref(xr, k.double(), v.double(), wq.double(), wp.double(), bp.double(), 4, 0.5, 3)
    out.backward(dout.double())
    assert R.rel_err(r["dx"], xr.grad) <= 1e-14
    assert R.rel_err(R.rank1_eval(x, k, v, wq, wp, bp, dout, 4, 0.5, 3, mutant="no_repsum")["dx"], xr.grad) > 0.1


# ---- what the input families promise ----------------------------------------------------------------------------------
SRA, GATE, RANK1 = R.sra_cases(), R.gate_cases(), R.rank1_cases()


@DT
@pytest.mark.parametrize("case", [c for c in SRA if c[1] == "selector"], ids=lambda c: c[0])
def test_selector_rows_are_one_hot_on_their_own_key(case, dtype):
    _, fam, B, heads, Nq, Nk, seed = case
    q, kv, _ = R.round_inputs(R.sra_inputs(fam, B, heads, Nq, Nk, seed), dtype)
    p = R.sra_logits(q, kv, heads, 0.125).softmax(-1)
    own = p[..., torch.arange(Nq), torch.arange(Nq) % Nk]
    assert float(own.min()) >= 0.99
    ref = R.sra_eval(q, kv, q, heads, 0.125)["o"].view(B, Nq, heads, 64)
    v = kv[..., heads * 64:].view(B, Nk, heads, 64)[:, torch.arange(Nq) % Nk].double()
    assert float((ref - v).abs().max()) <= 0.01 * 2 * float(v.abs().max())      # the output is the own key's value row


@DT
@pytest.mark.parametrize("case", [c for c in SRA if c[1].startswith("offset")], ids=lambda c: c[0])
def test_offset_rows_need_the_max_subtraction(case, dtype):
    _, fam, B, heads, Nq, Nk, seed = case
    q, kv, _ = R.round_inputs(R.sra_inputs(fam, B, heads, Nq, Nk, seed), dtype)
    s = R.sra_logits(q, kv, heads, 0.125)
    naive = torch.exp(s.float())
    if fam == "offset+":
        assert bool(torch.isinf(naive).all()) and abs(float(s.mean()) - 120.0) < 2.0
    else:
        assert bool((naive == 0).all()) and abs(float(s.mean()) + 120.0) < 2.0
    if Nk > 1:
        spread = s.amax(-1) - s.amin(-1)
        assert 0.0 < float(spread.max()) < 12.0                                     # the in-row spread stays O(1)


@DT
@pytest.mark.parametrize("case", [c for c in GATE if c[1] == "saturated"], ids=lambda c: c[0])
def test_saturated_gates_underflow(case, dtype):
    _, fam, heads, hd, T, B, qb, da, seed = case
    (q, k, v, dout, dattn), ref, _ = R.gate_setup(case, dtype)
    ns = (heads + 1) // 2
    qx = R.gate_expand(q.double(), B).view(B, T, heads, hd)
    s = ((qx * k.double().view(B, 1, heads, hd)).sum(-1) * hd ** -0.5)[..., :ns]
    assert float((s.abs() - 40.0).abs().max()) < 1.0
    g = ref["attn"].float()
    assert bool(((g * (1 - g)) == 0)[:, 0].any())


@DT
@pytest.mark.parametrize("case", [c for c in RANK1 if c[1] == "saturated"], ids=lambda c: c[0])
def test_saturated_rank1_gates_underflow(case, dtype):
    _, fam, C, T, xb, reps, wb, wd, seed = case
    (x, k, v, wq, wp, bp, dout), ref, _ = R.rank1_setup(case, dtype)
    s = R.rank1_logits(x, k, wq, 4, (C // 4) ** -0.5, reps)[..., :2]
    assert float((s.abs() - 40.0).abs().max()) < 2.0
    g = torch.sigmoid(s.float())
    assert bool(((g * (1 - g)) == 0)[..., 0].any())


def test_case_lists_cover_every_axis_value():
    assert {c[5] for c in SRA if c[1] == "gaussian" and c[2] == 2 and c[3] == 2} == set(R.SRA_NK)
    assert {c[4] for c in SRA} >= set(R.SRA_NQ)
    for fam in ("selector", "offset+", "offset-"):
        assert {c[5] for c in SRA if c[1] == fam and c[3] == 2} == {1, 17, 65, 129, 256}
    assert len(GATE) <= 60 and {(c[2], c[3]) for c in GATE} == set(R.GATE_HEADS) and {c[4] for c in GATE} == set(R.GATE_T)
    assert {(c[2], c[3], c[5], c[6]) for c in GATE} == {(h, d, b, q) for h, d in R.GATE_HEADS for b, q in R.GATE_BQ}
    assert {c[7] for c in GATE} == {True, False} and {c[1] for c in GATE} == {"gaussian", "saturated"}
    assert {c[2] for c in RANK1} == set(R.RANK1_C) and {c[3] for c in RANK1} == set(R.RANK1_T)
    assert {(c[4], c[5]) for c in RANK1} == set(R.RANK1_XR)
    for i in (1, 6, 7):
        assert {c[i] for c in RANK1} == ({"gaussian", "saturated"} if i == 1 else {True, False})
    # every mutant is live somewhere in its family
    assert {m for c in SRA for m in R.sra_mutants(c[1], c[4], c[5], BF)} == {"drop_last", "admit_zero", "swap_v", "rowmax16"}
    assert {m for c in GATE for m in R.gate_mutants(c[5], c[6])} == {"drop_token", "qbatch"}
    assert {m for c in RANK1 for m in R.rank1_mutants(c[5])} == {"drop_token", "no_repsum"}


# ---- mutants: for every GPU case, wrong float64 evaluations miss that case's bar ------------------------------------------
def _caught(mut, ref, cal, dtype, o_bound=None):
    r = R.ratios(mut, ref, cal, dtype, o_bound)
    return not R.within(r), r


@DT
@pytest.mark.parametrize("case", SRA, ids=lambda c: c[0])
def test_sra_mutants_miss_the_bar(case, dtype):
    _, fam, B, heads, Nq, Nk, seed = case
    (q, kv, dout), ref, cal, bound = R.sra_setup(case, dtype)
    assert R.within(R.ratios(R.sra_eval(q, kv, dout, heads, 0.125), ref, cal, dtype, bound))      # the reference itself passes
    for m in R.sra_mutants(fam, Nq, Nk, dtype):
        hit, r = _caught(R.sra_eval(q, kv, dout, heads, 0.125, mutant=m), ref, cal, dtype, bound)
        assert hit, (m, r)


@DT
@pytest.mark.parametrize("case", GATE, ids=lambda c: c[0])
def test_gate_mutants_miss_the_bar(case, dtype):
    _, fam, heads, hd, T, B, qb, da, seed = case
    (q, k, v, dout, dattn), ref, cal = R.gate_setup(case, dtype)
    for m in R.gate_mutants(B, qb):
        hit, r = _caught(R.gate_eval(q, k, v, dout, dattn, heads, hd ** -0.5, mutant=m), ref, cal, dtype)
        assert hit, (m, r)


@DT
@pytest.mark.parametrize("case", RANK1, ids=lambda c: c[0])
def test_rank1_mutants_miss_the_bar(case, dtype):
    _, fam, C, T, xb, reps, wb, wd, seed = case
    (x, k, v, wq, wp, bp, dout), ref, cal = R.rank1_setup(case, dtype)
    for m in R.rank1_mutants(reps):
        hit, r = _caught(R.rank1_eval(x, k, v, wq, wp, bp, dout, 4, (C // 4) ** -0.5, reps, mutant=m), ref, cal, dtype)
        assert hit, (m, r)
