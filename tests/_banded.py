"""Guard-banded device buffers for the float64 parity tests (test_gpu_attention_edges.py, test_gpu_bn_parity.py): every tensor handed
to a kernel is a 16-byte-aligned slice of a larger buffer.  Input bands (and the unused columns of a channel slice) are NaN, output
bands and unused columns carry a bit pattern that must survive the call; no output element may be non-finite."""
import torch

DEV = "cuda:0"
F32, BF = torch.float32, torch.bfloat16
GUARD = 64                                   # elements on either side: 128 / 256 bytes, the payload stays 16-byte aligned
PAT = {F32: (torch.int32, 0x5A5A5A5A), BF: (torch.int16, 0x5A5A)}


class Banded:
    """Tensors carved out of guard-banded buffers; `check` after the calls."""

    def __init__(self):
        self.outs = []

    def inp(self, t, dtype):
        if t is None:
            return None
        buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        view = buf[GUARD:GUARD + t.numel()].view(t.shape)
        view.copy_(t.to(dtype))
        assert view.data_ptr() % 16 == 0 and view.is_contiguous()
        return view

    def out(self, name, shape, dtype, fill):
        n = 1
        for s in shape:
            n *= s
        it, pat = PAT[dtype]
        buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        buf.view(it).fill_(pat)
        view = buf[GUARD:GUARD + n].view(shape)
        view.fill_(fill)
        assert view.data_ptr() % 16 == 0
        self.outs.append((name, buf, n, view, None))
        return view

    # ---- [rows][ld] channel slices: columns col0 .. col0 + C of a wider row (a concat buffer); ld = None is the dense tensor ------
    def inp_cols(self, t, dtype, ld=None, col0=0):
        if t is None or ld is None:
            return self.inp(t, dtype)
        rows, c = t.shape
        buf = torch.full((rows * ld + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        view = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, col0:col0 + c]
        view.copy_(t.to(dtype))
        assert view.data_ptr() % 16 == 0 and col0 + c <= ld
        return view

    def out_cols(self, name, rows, c, dtype, fill, ld=None, col0=0):
        if ld is None:
            return self.out(name, (rows, c), dtype, fill)
        it, pat = PAT[dtype]
        buf = torch.empty(rows * ld + 2 * GUARD, dtype=dtype, device=DEV)
        buf.view(it).fill_(pat)
        view = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, col0:col0 + c]
        view.fill_(fill)
        assert view.data_ptr() % 16 == 0 and col0 + c <= ld
        self.outs.append((name, buf, rows * ld, view, (rows, ld, col0, c)))
        return view

    def check(self):
        torch.cuda.synchronize()
        for name, buf, n, view, cols in self.outs:
            it, pat = PAT[buf.dtype]
            ints = buf.view(it)
            assert bool((ints[:GUARD] == pat).all()) and bool((ints[GUARD + n:] == pat).all()), f"{name}: guard band overwritten"
            if cols is not None:
                rows, ld, col0, c = cols
                body = ints[GUARD:GUARD + n].view(rows, ld)
                assert bool((body[:, :col0] == pat).all()) and bool((body[:, col0 + c:] == pat).all()), f"{name}: columns outside the slice overwritten"
            assert bool(torch.isfinite(view).all()), f"{name}: non-finite output"
