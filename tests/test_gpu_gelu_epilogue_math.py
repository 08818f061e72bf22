"""The GELU epilogue math (common.h: gelu_and_grad / gelu_fast on the hardware reciprocal and exponential) against float64
x * Phi(x) and Phi(x) + x * phi(x).  A 1x1 conv with a one-hot weight (Cin = Cout = 64, 256 rows) makes the pre-activation equal
to the bf16-exact input, so the epilogue sees chosen values: a grid over [-10, 10], +-0, +-40, +-1e4 and the neighbourhood of
the GELU minimum (-0.75)."""
import functools
import math

import pytest
import torch

from tests.test_gpu_ops import DEV, _check, _ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BIG = 10            # the 256x256 tile (bf16 only)
ROWS, C = 256, 64
SPECIAL = [0.0, -0.0, 40.0, -40.0, 1e4, -1e4]


@functools.lru_cache(maxsize=None)
def _problem():
    """[ROWS, C] bf16-exact inputs + float64 references, built once and never modified"""
    n = ROWS * C
    near_min = torch.linspace(-0.77, -0.73, 64)
    grid = torch.linspace(-10.0, 10.0, n - len(SPECIAL) - near_min.numel())
    x = torch.cat([torch.tensor(SPECIAL), near_min, grid]).to(BF).float()
    x64 = x.double()
    cdf = 0.5 * torch.erfc(-x64 / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x64 * x64) / math.sqrt(2.0 * math.pi)
    return dict(x=x.view(ROWS, C), y=(x64 * cdf).view(ROWS, C), d=(cdf + x64 * pdf).view(ROWS, C))


def _compare(got_y, got_d, dtype, what):
    e = _problem()
    x = e["x"]
    gy = got_y.float().cpu().view(ROWS, C)
    outs = [("y", gy, e["y"])]
    if got_d is not None:
        outs.append(("aux", got_d.float().cpu().view(ROWS, C), e["d"]))
    core, mid = x.abs() <= 10.0, x.abs() <= 6.0
    for name, g, ref in outs:
        assert torch.isfinite(g).all(), f"{what} {name}: non-finite output"
        err = (g.double() - ref).abs()
        print(f"gelu math {what} {name}: max err |x|<=6 {float(err[mid].max()):.3e}, |x|<=10 {float(err[core].max()):.3e}, "
              f"all {float(err.max()):.3e}")
        # _check's bars (2e-5 f32 / 1.2e-2 bf16, of max(1, max|ref|)): on the grid alone - the +-1e4 inputs would widen the bar of a
        # joint check to 0.2 - and on everything
        sel = core.view(-1)
        _check(g.view(-1)[sel], ref.view(-1)[sel].float(), dtype, f"{what} {name} on [-10, 10]")
        _check(g, ref.float(), dtype, f"{what} {name}")
        if dtype == torch.float32:
            # 1.5e-7 (Abramowitz-Stegun 7.1.26) + one ulp each from the reciprocal and the exponential, through a polynomial
            # bounded by 1 on t in (0, 1]
            assert float(err[mid].max()) <= 5e-7, f"{what} {name}: {float(err[mid].max()):.3e} for |x| <= 6"
    # far tails: gelu(-40) = gelu(-1e4) = +-0 with derivative 0; gelu(x) = x and gelu' = 1 at +40, +1e4
    flat_x, flat_y = x.view(-1), gy.view(-1)
    for i in range(len(SPECIAL)):
        v = float(flat_x[i])   # (1e4 is 9984 in bf16)
        if v <= -40.0:
            assert float(flat_y[i]) == 0.0, (what, v, float(flat_y[i]))
        if v >= 40.0:
            assert float(flat_y[i]) == v, (what, v, float(flat_y[i]))
        if got_d is not None and abs(v) >= 40.0:
            assert float(outs[1][1].view(-1)[i]) == (0.0 if v < 0 else 1.0), (what, v)
    assert float(flat_y[0]) == 0.0 and float(flat_y[1]) == 0.0


@pytest.mark.parametrize("tile,dtype", [(0, torch.float32), (1, torch.float32), (0, BF), (1, BF), (BIG, BF)],
                         ids=["tile0-f32", "tile1-f32", "tile0-bf16", "tile1-bf16", "big-bf16"])
def test_fc1_gelu_epilogue_with_derivative(tile, dtype):
    """aux_mode 1: y = gelu(x), aux = gelu'(x) (gelu_and_grad)"""
    ops = _ops()
    e = _problem()
    xv = e["x"].to(dtype).to(DEV).view(1, 1, ROWS, C)
    wp = ops.pack_weight(torch.eye(C).view(C, C, 1, 1).contiguous().to(DEV), dtype)
    y = torch.full((1, 1, ROWS, C), float("nan"), dtype=dtype, device=DEV)
    d = torch.full_like(y, float("nan"))
    ops.conv2d(xv, wp, y, act=ops.ACT_GELU, aux=d, aux_mode=1, tile=tile)
    torch.cuda.synchronize()
    _compare(y, d, dtype, f"aux_mode1 tile{tile}")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_linear_gelu(dtype):
    """ops.linear(act=ACT_GELU): gelu_fast for bf16 outputs, erff for f32"""
    ops = _ops()
    e = _problem()
    xv = e["x"].to(dtype).to(DEV).view(1, ROWS, C)
    wp = ops.pack_weight(torch.eye(C).contiguous().to(DEV), dtype)
    y = torch.full((1, ROWS, C), float("nan"), dtype=dtype, device=DEV)
    ops.linear(xv, wp, y, act=ops.ACT_GELU)
    torch.cuda.synchronize()
    _compare(y, None, dtype, "linear")
