"""CPU half of the integer-lattice parity tests (tests/_lattice.py): the generators keep their ranges, every case of
test_gpu_exact_conv.py / test_gpu_exact_grad.py meets its 2^24 precondition and - for bf16 outputs - the magnitude condition, float32
arithmetic on the CPU is bit-equal to float64 on such inputs, and a mutation table records the gap the exact comparison closes: each
mutation of a reference is rejected by assert_exact and accepted by the tolerance checks of test_gpu_ops / test_gpu_train_ops."""
import pytest
import torch
import torch.nn.functional as F

from tests import _lattice as L
from tests import test_gpu_exact_conv as EC
from tests import test_gpu_exact_grad as EG
from tests.test_gpu_ops import CONV_CASES, _check as check_ops
from tests.test_gpu_train_ops import CONV, _check as check_train

BF = torch.bfloat16


def _vals(t):
    return set(t.unique().tolist())


def test_generators_keep_their_ranges():
    for K in (64, 576, 2736, 4096, 12288):
        x = L.activations((64, K), K, 1)
        assert _vals(x) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        p = L.keep_probability(K)
        share = float((x != 0).float().mean())
        assert abs(share - 0.8 * p) < 0.02, (K, share, p)     # 4 of the 5 lattice values are non-zero
        assert K * 2 * 1 < L.EXACT_LIMIT
    assert _vals(L.weights((64, 99), 2)) == {-1.0, 1.0}
    assert _vals(L.out_grads((4, 8, 9, 9), 72, 3)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert _vals(L.pow2_scales(4096, 4)) == {0.25, 0.5, 1.0, 2.0, 4.0}
    assert _vals(L.ints((4096,), -8, 8, 5)) == set(float(v) for v in range(-8, 9))
    assert torch.equal(L.activations((5, 7), 64, 9), L.activations((5, 7), 64, 9)), "seeded"
    x, wt = L.biased_conv_inputs(1, 256, 6, 6, 32, 3, 6)
    assert _vals(x) == {0.0, 1.0, 2.0} and _vals(wt) == {-1.0, 1.0}


def test_reference_std_stays_inside_the_bf16_integer_range():
    for K in (64, 576, 2736, 4096, 12288):
        x, w = L.activations((512, K), K, 10), L.weights((256, K), 11)
        y = L.ref64_linear(x, w)
        assert float(y.std()) <= 48.5 and L.share_above(y) == 0.0, (K, float(y.std()), float(y.abs().max()))
        assert torch.equal((x @ w.t()).double(), y), "f32 matmul == float64"
        assert torch.equal((x.to(BF).float() @ w.to(BF).float().t()).double(), y), "bf16 storage loses nothing"


def test_bf16_ties_round_to_even():
    t = torch.tensor([257.0, 259.0, 261.0, 263.0, 514.0, 518.0, -257.0], dtype=torch.float64)
    assert L.expected(t, BF).float().tolist() == [256.0, 260.0, 260.0, 264.0, 512.0, 520.0, -256.0]
    assert L.truncate_to_bf16(t).float().tolist() == [256.0, 258.0, 260.0, 262.0, 512.0, 516.0, -256.0]


@pytest.mark.parametrize("case", [CONV[1], CONV[3], CONV[7], CONV[9], CONV[12]], ids=lambda c: c[0])
def test_cpu_f32_conv_dgrad_wgrad_equal_float64(case):
    name, n, h, w, cin, cout, k, s, p, d = case
    pb = EG.grad_inputs(name)
    x, wt = pb["x"].clone().requires_grad_(True), pb["w"].clone().requires_grad_(True)
    y = F.conv2d(x, wt, None, s, p, d)
    y.backward(pb["dy"])
    assert torch.equal(y.detach().double(), L.ref64_conv(pb["x"], pb["w"], s, p, d))
    assert torch.equal(x.grad.double(), L.ref64_dgrad(pb["dy"], pb["w"], pb["x"].shape, s, p, d))
    dw, db = L.ref64_wgrad(pb["x"], pb["dy"], pb["w"].shape, s, p, d)
    assert torch.equal(wt.grad.double(), dw) and torch.equal(pb["dy"].sum((0, 2, 3)).double(), db)


def test_preconditions_are_enforced():
    x, w = L.activations((1, 8, 4, 4), 8, 1), L.weights((8, 8, 1, 1), 2)
    with pytest.raises(AssertionError):
        L.ref64_conv(x * 0.3, w)                                      # off the lattice
    with pytest.raises(AssertionError):
        L.ref64_conv(x, w, scale=torch.full((8,), 3.0))               # not a power of two
    with pytest.raises(AssertionError):
        L.ref64_conv(x, w, scale=torch.full((8,), 8.0))               # outside [1/4, 4]
    with pytest.raises(AssertionError):
        L.ref64_conv(x, w, shift=torch.full((8,), 2.0 ** 23))         # leaves the exact range
    with pytest.raises(AssertionError):
        L.bf16_magnitude_ok(torch.full((10,), 300.0, dtype=torch.float64), "all above 256")
    with pytest.raises(AssertionError):
        L._act64(torch.zeros(1, dtype=torch.float64), 3)   # GELU is not exact on integers


_BF16_CASES = EC.bf16_reference_cases() + EG.bf16_reference_cases()


@pytest.mark.parametrize("name,make", _BF16_CASES, ids=[c[0] for c in _BF16_CASES])
def test_bf16_output_case_meets_the_magnitude_condition(name, make):
    """building the reference also runs the case's lattice / 2^24 asserts (ref64_* wrappers)"""
    ref = make()
    assert ref.dtype == torch.float64
    L.bf16_magnitude_ok(ref, name)


_WGRAD_CASES = EG.wgrad_input_cases()


@pytest.mark.parametrize("name,make", _WGRAD_CASES, ids=[c[0] for c in _WGRAD_CASES])
def test_wgrad_case_stays_exact_in_f32(name, make):
    x, dy, rows = make()
    assert _vals(x) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and _vals(dy) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert rows * 2 * 2 + 3 < L.EXACT_LIMIT


def test_shape_tables_are_the_suites_own():
    assert all(c[0] in EC.FWD_TABLE and EC.FWD_TABLE[c[0]] is c for c in CONV_CASES)
    assert all(c[0] in EG.GRAD_TABLE and EG.GRAD_TABLE[c[0]] is c for c in CONV)
    assert set(EC.TILES) | {EC.BIG_TILE} == set(range(15))


def test_probe_reaches_the_tie_range():
    pb = EC.probe_problem()
    EC.probe_preconditions(pb)
    ref = pb["conv"]
    assert int((L.expected(ref, BF) != L.truncate_to_bf16(ref)).sum()) >= 1000
    assert float(ref.abs().max()) <= 2048


def test_assert_exact_locates_the_mismatch():
    ref = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).view(2, 3, 4, 5)
    L.assert_exact(ref.float(), ref, torch.float32, "identity", "nhwc")
    L.assert_exact(ref.to(BF), ref, BF, "identity", "nhwc")
    got = ref.float().clone()
    got[1, 2, 0, 3] += 1
    got[1, 2, 3, 4] -= 2
    with pytest.raises(AssertionError) as e:
        L.assert_exact(got, ref, torch.float32, "two wrong", "nhwc")
    msg = str(e.value)
    assert "2 of 120" in msg and "n=1, h=2, w=0, c=3" in msg and "got 104.0, want 103.0" in msg and "= 2.0 at (1, 2, 3, 4)" in msg
    got = ref.float().clone()
    got[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        L.assert_exact(got, ref, torch.float32, "nan", "nhwc")


# ---- mutation table ---------------------------------------------------------------------------------------------------------------
def _rejected(got, ref64, dtype, what):
    with pytest.raises(AssertionError):
        L.assert_exact(got, ref64, dtype, what)


def test_mutation_one_term_dropped_from_every_sum():
    """3x3_cin304_ktail in bf16: every output loses its (channel 0, centre tap) product, |error| <= 2; the tolerance is ~2.5"""
    pb = EC.fwd_problem("3x3_cin304_ktail")
    ref = pb["ref"].permute(0, 3, 1, 2)
    mut = ref - F.conv2d(pb["x"][:, :1].double(), pb["w"][:, :1, 1:2, 1:2].double())
    assert float((mut != ref).double().mean()) > 0.2
    _rejected(mut.to(BF), ref, BF, "dropped term")
    check_ops(mut.to(BF), ref.float(), BF, "dropped term")


def test_mutation_one_pixel_row_dropped_from_a_wgrad():
    """6272 x 256 -> 304 linear weight gradient from bf16 operands: pixel row 100 never added; max |dw| is several hundred, the
    tolerance 2e-2 of that"""
    x, dy = EG.linear_wgrad_inputs(EG.LINEAR_WGRAD[3])
    dw, _ = L.ref64_linear_wgrad(x, dy)
    mut = dw - torch.outer(dy[100].double(), x[100].double())
    assert float((mut != dw).double().mean()) > 0.2
    _rejected(mut.float(), dw, torch.float32, "dropped row")
    check_train(mut.float(), dw.float(), BF, "dropped row", f32_tol=5e-5, bf16_tol=2e-2)


def test_mutation_accumulator_rounded_before_the_residual():
    pb = EC.probe_problem()
    ref = pb["conv"] + pb["small"]
    mut = L.expected(pb["conv"], BF).double() + pb["small"]
    _rejected(mut.to(BF), ref, BF, "early rounding")
    assert int((mut.to(BF) != L.expected(ref, BF)).sum()) >= 1000
    check_ops(mut.to(BF), ref.float(), BF, "early rounding")
    # and with the cancelling residual of the GPU probe the rounded accumulator leaves nothing at all
    assert float((L.expected(pb["conv"], BF).double() + pb["res"]).abs().max()) == 0.0


def test_mutation_truncation_instead_of_rne():
    ref = EC.probe_problem()["conv"]
    mut = L.truncate_to_bf16(ref)
    _rejected(mut, ref, BF, "truncation")
    check_ops(mut, ref.float(), BF, "truncation")


def test_mutation_one_element_off_by_one():
    pb = EC.fwd_problem("3x3_cin304_ktail")
    ref = pb["ref"]
    mut = ref.clone()
    idx = tuple(int(v) for v in torch.nonzero(ref.abs() < 100)[12345])
    mut[idx] += 1
    _rejected(mut.to(BF), ref, BF, "off by one")
    assert int((mut.to(BF) != L.expected(ref, BF)).sum()) == 1
    check_ops(mut.to(BF).permute(0, 3, 1, 2), ref.permute(0, 3, 1, 2).float(), BF, "off by one")
