"""Integer-lattice inputs for which the conv / GEMM kernels have ONE correct answer, bit for bit.

With activations in {-2..2}, weights in {-1, +1} and K * 2 < 2^24 every product and every partial sum is an integer that float32
represents exactly: MFMA accumulators, split-K partials, f32 atomics and fixed-order finishes all give the number float64 gives on the
CPU, in any summation order.  An f32 output must then be torch.equal to the float64 reference; a bf16 output must equal
ref.to(bfloat16), one round-to-nearest-even of an exact value.  There is no tolerance: a dropped, duplicated or misplaced term moves
an integer by at least 1.

Above |y| = 256 bf16 no longer holds every integer, so a unit error could hide in the rounding: activations are thinned with
keep-probability min(1, 2304 / (2 K)) (the reference's std stays near 48 for every K) and bf16_magnitude_ok() holds each bf16-output
case to at most 0.1 % of elements above 256.  biased_conv_inputs() goes the other way on purpose (results in 256..2048) for the
tie-rounding and early-rounding probes.

Helper module (not a conftest): imported by test_lattice_host.py, test_gpu_exact_conv.py, test_gpu_exact_grad.py and
tools/fuzz_conv.py --exact."""
import math

import torch
import torch.nn.functional as F

EXACT_LIMIT = float(1 << 24)     # integers up to here are exact in float32
BF16_INT_LIMIT = 256.0           # ... and up to here in bfloat16
MAX_SHARE_ABOVE = 1e-3
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
LEAKY_SLOPE = 0.01


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def keep_probability(K, gain=1.0):
    """share of non-zero-able activations for a reduction of length K; gain = the largest |scale| applied to the sum afterwards."""
    return min(1.0, 2304.0 / (2.0 * K * gain * gain))


def ints(shape, lo, hi, seed):
    """uniform integers in [lo, hi] as float32"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).float()


def activations(shape, K, seed, gain=1.0, thin=True):
    """{-2..2}, thinned to keep the reduction over K terms (times gain) inside the bf16 integer range"""
    g = _gen(seed)
    v = torch.randint(-2, 3, tuple(shape), generator=g).float()
    p = keep_probability(K, gain) if thin else 1.0
    if p < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < p).float()
    return v


def weights(shape, seed):
    """{-1, +1}"""
    return torch.randint(0, 2, tuple(shape), generator=_gen(seed)).float() * 2.0 - 1.0


def out_grads(shape, K, seed):
    """output gradients in {-2..2}; K = the data gradient's reduction length (Cout * kh * kw)"""
    return activations(shape, K, seed)


def pow2_scales(n, seed):
    """powers of two in [1/4, 4]"""
    return torch.pow(2.0, torch.randint(-2, 3, (n,), generator=_gen(seed)).float())


def biased_conv_inputs(n, cin, h, w, cout, k, seed):
    """(x, wt) whose convolution lands in +-(256..2048): x in {0, 1, 2}, and output channel o has its weights +1 with probability
    1/2 +- b_o, so its sums centre on +-2 b_o K.  Integers above 256: odd ones are bf16 ties in 256..512, n % 4 == 2 in 512..1024."""
    g = _gen(seed)
    K = cin * k * k
    x = torch.randint(0, 3, (n, cin, h, w), generator=g).float()
    lo, hi = 330.0 / (2.0 * K), min(0.45, 1800.0 / (2.0 * K))
    assert lo < hi, "reduction too short to reach the bf16 tie range"
    b = torch.linspace(lo, hi, cout) * (torch.arange(cout) % 2 * 2 - 1).float()
    wt = (torch.rand((cout, cin, k, k), generator=g) < (0.5 + b)[:, None, None, None]).float() * 2.0 - 1.0
    return x, wt


def _amax(t):
    return 0.0 if t is None or t.numel() == 0 else float(t.abs().max())


def conv_bound(K, x, w, scale=None, shift=None, nbias=None, residual=None):
    """largest magnitude any intermediate of act((conv + nbias) * scale + shift + residual) can reach"""
    s = max(1.0, _amax(scale)) if scale is not None else 1.0
    return (K * _amax(x) * _amax(w) + _amax(nbias)) * s + _amax(shift) + _amax(residual)


def _is_lattice(t, denom=1.0):
    return t is None or bool((t.double() * denom == (t.double() * denom).round()).all())


def _act64(y, act):
    if act == ACT_RELU:
        return y.relu()
    if act == ACT_LEAKY:   # one f32 multiply of an exact value: the CPU does the same multiply in f32
        return F.leaky_relu(y.float(), LEAKY_SLOPE).double()
    assert act == ACT_NONE, "only activations that are exact on integers belong here"
    return y


def ref64_conv(x, w, stride=1, pad=0, dil=1, scale=None, shift=None, nbias=None, residual=None, act=ACT_NONE, stride_w=0):
    """float64 act((conv(x, w) + nbias[n]) * scale + shift + residual); x [N,Cin,H,W], w [Cout,Cin,kh,kw], residual NCHW of the
    output's shape.  Exact: asserts that every operand is on the lattice and that no intermediate can leave the f32 integer range."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    assert _is_lattice(x) and _is_lattice(w) and _is_lattice(shift) and _is_lattice(nbias) and _is_lattice(residual)
    if scale is not None:
        l2 = torch.log2(scale.double())
        assert bool((l2 == l2.round()).all()) and float(l2.abs().max()) <= 2, "scales must be powers of two in [1/4, 4]"
    bound = conv_bound(K, x, w, scale, shift, nbias, residual)
    assert bound * 4 < EXACT_LIMIT, f"precondition: {bound} * 4 (quarter steps) must stay below 2^24"
    y = F.conv2d(x.double(), w.double(), None, (stride, stride_w or stride), pad, dil)
    if nbias is not None:
        y = y + nbias.double()[:, :, None, None]
    if scale is not None:
        y = y * scale.double()[None, :, None, None]
    if shift is not None:
        y = y + shift.double()[None, :, None, None]
    if residual is not None:
        y = y + residual.double()
    return _act64(y, act)


def ref64_linear(x, w, bias=None, act=ACT_NONE):
    """float64 act(x @ w^T + bias); x [rows, Cin], w [Cout, Cin]"""
    assert _is_lattice(x) and _is_lattice(w) and _is_lattice(bias)
    bound = w.shape[1] * _amax(x) * _amax(w) + _amax(bias)
    assert bound < EXACT_LIMIT, f"precondition: {bound} must stay below 2^24"
    y = x.double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()[None]
    return _act64(y, act)


def ref64_dgrad(dy, w, x_shape, stride=1, pad=0, dil=1, residual=None):
    """float64 data gradient of conv(x, w) for the output gradient dy (+ residual, a gradient the input already holds)"""
    assert _is_lattice(dy) and _is_lattice(w) and _is_lattice(residual)
    K = w.shape[0] * w.shape[2] * w.shape[3]
    bound = K * _amax(dy) * _amax(w) + _amax(residual)
    assert bound < EXACT_LIMIT, f"precondition: {bound} must stay below 2^24"
    dx = torch.nn.grad.conv2d_input(tuple(x_shape), w.double(), dy.double(), stride, pad, dil)
    return dx if residual is None else dx + residual.double()


def ref64_wgrad(x, dy, w_shape, stride=1, pad=0, dil=1, prior=None):
    """float64 weight gradient [Cout,Cin,kh,kw] (+ prior, the gradient the destination already holds) and the bias gradient [Cout]"""
    assert _is_lattice(x) and _is_lattice(dy) and _is_lattice(prior)
    rows = dy.shape[0] * dy.shape[2] * dy.shape[3]
    bound = rows * max(1.0, _amax(x)) * _amax(dy) + _amax(prior)
    assert bound < EXACT_LIMIT, f"precondition: {bound} must stay below 2^24"
    if w_shape[2] == 1 and w_shape[3] == 1 and stride == 1 and pad == 0:
        dw = (dy.double().permute(1, 0, 2, 3).reshape(w_shape[0], -1) @ x.double().permute(0, 2, 3, 1).reshape(-1, w_shape[1]))
        dw = dw.view(*w_shape)
    else:
        dw = torch.nn.grad.conv2d_weight(x.double(), tuple(w_shape), dy.double(), stride, pad, dil)
    db = dy.double().sum(dim=(0, 2, 3))
    return (dw if prior is None else dw + prior.double()), db


def ref64_linear_wgrad(x, dy):
    """float64 dy^T x [Cout, Cin] and the column sums of dy"""
    assert _is_lattice(x) and _is_lattice(dy)
    bound = x.shape[0] * max(1.0, _amax(x)) * _amax(dy)
    assert bound < EXACT_LIMIT, f"precondition: {bound} must stay below 2^24"
    return dy.double().t() @ x.double(), dy.double().sum(0)


def share_above(ref64, limit=BF16_INT_LIMIT):
    return float((ref64.abs() > limit).double().mean())


def bf16_magnitude_ok(ref64, what):
    """the magnitude condition of a bf16-output case, asserted on the reference alone (before any kernel runs)"""
    share = share_above(ref64)
    assert share <= MAX_SHARE_ABOVE, f"{what}: {share:.2e} of the reference exceeds {BF16_INT_LIMIT:.0f} (a unit error could hide in bf16)"


def expected(ref64, dtype):
    """what the kernel must store: the exact value, rounded once (to nearest even) for bf16"""
    if dtype == torch.float32:
        return ref64.float()
    assert dtype == torch.bfloat16
    return ref64.float().to(torch.bfloat16)


def truncate_to_bf16(t):
    """round-toward-zero to bf16 (the mutation a correct kernel must not make)"""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def assert_exact(got, ref64, dtype, what, axes=None):
    """got (any device, dtype `dtype`) == expected(ref64, dtype), element for element.  On failure: the number of mismatches, the
    first mismatching index (named by `axes`, e.g. "nhwc" or "oikk"), got / want there, and the largest difference."""
    want = ref64 if ref64.dtype == dtype else expected(ref64, dtype)
    got = got.detach().cpu()
    assert got.dtype == dtype, (what, got.dtype, dtype)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    g, w_ = got.double(), want.double()
    bad = (g != w_) | torch.isnan(g)
    idx = torch.nonzero(bad)
    first = tuple(int(v) for v in idx[0])
    names = axes if axes is not None and len(axes) == got.dim() else None
    where = ", ".join(f"{names[i]}={v}" for i, v in enumerate(first)) if names else str(first)
    diff = (g - w_).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, math.inf), diff)
    worst = tuple(int(v) for v in torch.nonzero(diff == diff.max())[0])
    lo = [int(v) for v in idx.min(0).values]
    hi = [int(v) for v in idx.max(0).values]
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({str(dtype)[6:]}); first at ({where}): got {float(g[first])!r}, "
        f"want {float(w_[first])!r}; largest |got - want| = {float(diff.max())!r} at {worst}; mismatches span {lo} .. {hi}")
