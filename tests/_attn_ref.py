"""float64 references, rounding-point models, input families, mutants and the case lists of the three attention families
(SRA softmax attention: csrc/pvt_ops.hip + pvt_train.hip; the attention gate: csrc/attn_gate.hip; the one-key collapse:
csrc/attn_rank1.hip).  CPU only; shared by test_attn_ref_host.py (no GPU) and test_gpu_attention_edges.py.

Every evaluation takes `model`: None is the reference (torch.float64); "f32" is the same formula in PyTorch's f32 CPU arithmetic;
"bf16" is f32 arithmetic with tensors rounded to bf16 where the kernels store or pack bf16.  The models only calibrate bars
(how far a correct evaluation in that arithmetic sits from float64); nothing is ever compared against them.

Error measure everywhere: max |got - ref| / max |ref| of that output (`rel_err`).  Bars (`ratios`):
  f32:   err <= max(4 * e32, 1e-6), e32 = rel_err of model "f32";
  bf16:  err <= 3 * e_bf16, e_bf16 = rel_err of model "bf16"; the SRA forward output instead has the derived element-wise bound
         |o - ref| <= 1.5 * 2 * 2^-9 * Vmax(batch item, head)."""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
F32_MAX = float(torch.finfo(F32).max)


def _rb(t):
    """round to bf16, keep the carrier dtype"""
    return t.to(BF).to(t.dtype)


def _arith(model):
    """(dtype of the arithmetic, rounding applied where the kernels hold bf16)"""
    if model is None:
        return F64, (lambda t: t)
    if model == "f32":
        return F32, (lambda t: t)
    if model == "bf16":
        return F32, _rb
    raise ValueError(model)


def rel_err(got, ref):
    ref = ref.detach().to(F64)
    d = float((got.detach().to(F64) - ref).abs().max()) if ref.numel() else 0.0
    den = float(ref.abs().max()) if ref.numel() else 0.0
    if den > 0.0:
        return d / den
    return 0.0 if d == 0.0 else math.inf     # (NaN stays NaN: `nan <= bar` is False)


# ---- SRA softmax attention --------------------------------------------------------------------------------------------
def _split_heads(q, kv, heads):
    B, Nq, C = q.shape
    Nk, hd = kv.shape[1], C // heads
    qh = q.view(B, Nq, heads, hd).permute(0, 2, 1, 3)
    kh = kv[..., :C].reshape(B, Nk, heads, hd).permute(0, 2, 1, 3)
    vh = kv[..., C:].reshape(B, Nk, heads, hd).permute(0, 2, 1, 3)
    return qh, kh, vh


def sra_ref(q, kv, heads, scale):
    """pvt.py:102-130 in the dtype of its inputs (autograd-friendly): softmax(scale q k^T) v per head."""
    B, Nq, C = q.shape
    qh, kh, vh = _split_heads(q, kv, heads)
    return (((qh @ kh.transpose(-2, -1)) * scale).softmax(-1) @ vh).transpose(1, 2).reshape(B, Nq, C)


def sra_grads_autograd(q, kv, dout, heads, scale):
    """float64 autograd of sra_ref: {o, dq, dkv}."""
    qr, kvr = q.to(F64).clone().requires_grad_(True), kv.to(F64).clone().requires_grad_(True)
    o = sra_ref(qr, kvr, heads, scale)
    o.backward(dout.to(F64))
    return {"o": o.detach(), "dq": qr.grad, "dkv": kvr.grad}


def sra_eval(q, kv, dout, heads, scale, model=None, mutant=None):
    """{o, dq, dkv} by the explicit formulas the kernels use (test_attn_ref_host.py holds them to float64 autograd):
         S = scale Q K^T, e = exp(S - rowmax), P = e / sum e, O = P V,
         dP = dO V^T, delta = sum_key P dP, dS = scale P (dP - delta), dQ = dS K, dK = dS^T Q, dV = P^T dO.
    bf16 model: inputs are bf16; e is rounded before e V and normalised by the unrounded sum, O is rounded (pvt_ops.hip); dS is
    rounded before dS K and dS^T Q, P before P^T dO, dQ is rounded, dK / dV stay f32 (pvt_train.hip).
    mutant (float64 only): "drop_last", "admit_zero", "swap_v", "rowmax16"."""
    dt, rnd = _arith(model)
    q, kv, dout = rnd(q.to(dt)), rnd(kv.to(dt)), rnd(dout.to(dt))
    B, Nq, C = q.shape
    Nk = kv.shape[1]
    if mutant == "admit_zero":     # key Nk - a zero row of the staged tile - takes part in the softmax
        kv = torch.cat((kv, torch.zeros((B, 1, 2 * C), dtype=dt)), 1)
    if mutant == "swap_v":         # keys 0 and Nk - 1 trade places in V only
        v = kv[..., C:].clone()
        v[:, [0, Nk - 1]] = v[:, [Nk - 1, 0]]
        kv = torch.cat((kv[..., :C], v), -1)
    qh, kh, vh = _split_heads(q, kv, heads)
    doh = dout.view(B, Nq, heads, C // heads).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-2, -1)) * scale
    if mutant == "drop_last":      # the last key masked out like padding
        s[..., Nk - 1] = -math.inf
    m = s[..., :16].amax(-1, keepdim=True) if mutant == "rowmax16" else s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    if mutant == "rowmax16":       # what f32 exp does with the row's true maximum left above the subtracted one
        e = torch.where(e > F32_MAX, torch.full_like(e, math.inf), e)
    if mutant == "drop_last" and Nk == 1:
        e = torch.zeros_like(s)    # no key left
        den = torch.ones_like(m)
    else:
        den = e.sum(-1, keepdim=True)
    o = rnd((rnd(e) @ vh) / den)
    p = e / den
    dp = doh @ vh.transpose(-2, -1)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = rnd(p * (dp - delta) * scale)
    dq = rnd(ds @ kh)
    dk, dv = ds.transpose(-2, -1) @ qh, rnd(p).transpose(-2, -1) @ doh
    back = lambda t, n: t.permute(0, 2, 1, 3).reshape(B, n, C)
    dkv = torch.cat((back(dk, kh.shape[2]), back(dv, kh.shape[2])), -1)[:, :Nk]
    return {"o": back(o, Nq), "dq": back(dq, Nq), "dkv": dkv.contiguous()}


def sra_inputs(family, B, heads, Nq, Nk, seed):
    """(q, kv, dout) f32, head_dim 64, scale 1/8; distinct data per head and per batch item."""
    g = torch.Generator().manual_seed(seed)
    hd, C = 64, heads * 64
    q, kv, dout = (torch.randn(s, generator=g) for s in ((B, Nq, C), (B, Nk, 2 * C), (B, Nq, C)))
    k = kv[..., :C].reshape(B, Nk, heads, hd)
    if family == "selector":
        # keys of norm sqrt(32) per head: the own logit of query i = 4 k[i % Nk] is 0.125 * 4 * 32 = 16, every other one
        # 16 cos(angle) ~ N(0, 2^2): rows with 1 - p_own between ~1e-6 and ~1e-3, so the gradients (which vanish with 1 - p_own)
        # stay well above f32 rounding.  Where a key beyond the first 16 is selected, the last selected one is made orthogonal to
        # all others and given norm 15: its query's row is 112.5 against zeros - more than f32 exp absorbs (e^88.7) unless the
        # maximum that is subtracted is the row's own.
        nrm = lambda t: t.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        k = k * (32.0 ** 0.5 / nrm(k))
        jb = min(Nq, Nk) - 1
        if jb >= 16:
            kb = k[:, jb] / nrm(k[:, jb])                       # [B, heads, hd]
            k = k - (k * kb[:, None]).sum(-1, keepdim=True) * kb[:, None]
            k = k * (32.0 ** 0.5 / nrm(k))
            k[:, jb] = 15.0 * kb
        q = 4.0 * k[:, torch.arange(Nq) % Nk].reshape(B, Nq, C)
    elif family in ("offset+", "offset-"):
        # shared unit direction w per head; q0, k0 orthogonal to it: logit = 0.125 (q0 . k0 + a b) = O(1) +- 120
        w = torch.full((hd,), hd ** -0.5)
        a = math.sqrt(960.0)
        qh = q.view(B, Nq, heads, hd)
        qh = qh - (qh @ w)[..., None] * w + a * w
        k = k - (k @ w)[..., None] * w + (a if family == "offset+" else -a) * w
        q = qh.reshape(B, Nq, C)
    elif family != "gaussian":
        raise ValueError(family)
    kv = torch.cat((k.reshape(B, Nk, C), kv[..., C:]), -1).contiguous()
    return q.contiguous(), kv, dout


def sra_logits(q, kv, heads, scale):
    qh, kh, _ = _split_heads(q.to(F64), kv.to(F64), heads)
    return (qh @ kh.transpose(-2, -1)) * scale      # [B, heads, Nq, Nk]


SRA_NK = (1, 4, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 191, 193, 255, 256)
SRA_NQ = (1, 17, 64, 65, 130)


def sra_cases():
    """(id, family, B, heads, Nq, Nk, seed)"""
    out = []
    nq_of = {nk: SRA_NQ[i % len(SRA_NQ)] for i, nk in enumerate(SRA_NK)}
    for nk in SRA_NK:
        out.append((f"gaussian-nk{nk}-nq{nq_of[nk]}", "gaussian", 2, 2, nq_of[nk], nk, 1000 + nk))
    for fam in ("selector", "offset+", "offset-"):
        for nk in (1, 17, 65, 129, 256):
            out.append((f"{fam}-nk{nk}-nq{nq_of[nk]}", fam, 2, 2, nq_of[nk], nk, 2000 + nk))
    for fam in ("gaussian", "selector"):   # more than one query block per workgroup (cavp_sra_blocks_per_wg, common.h)
        out.append((f"{fam}-qpw2", fam, 2, 8, 2117, 17, 3001))
        out.append((f"{fam}-qpw3", fam, 1, 16, 4101, 5, 3002))
    return out


def sra_mutants(family, Nq, Nk, dtype=F32):
    """The mutants that change the function at this case by more than the arithmetic of `dtype` resolves (the others are the
    same function there): a zero-logit key is invisible next to logits of +120 (weight e^-120) and below the f32 floor next to a selector row's own
    logit of 16 (e^-16 = 1e-7); among N(0, 1) logits it
    weighs ~1 / (1.65 Nk + 1), which bf16 (2^-8 per stored value) resolves for certain only up to Nk = 16 (3.6 %) - beyond, the
    f32 run of the same case and the bf16 offset- cases (where the admitted key takes the whole row) carry that mutant; a key
    no query selects has weight ~e^-16 in the selector family; the row maximum only matters to f32 exp when the true one
    exceeds the subtracted one by > 88, which takes a selected key beyond the first 16; one key cannot be swapped."""
    out = []
    if family != "selector" or Nk - 1 < Nq:
        out.append("drop_last")
    if family == "offset-" or (family == "gaussian" and (dtype == F32 or Nk <= 16)):
        out.append("admit_zero")
    if Nk >= 2:
        out.append("swap_v")
    if family == "selector" and min(Nq, Nk) > 16:
        out.append("rowmax16")
    return out


# ---- attention gate ---------------------------------------------------------------------------------------------------
def gate_ref(q, k, v, heads, scale, q_batch):
    """attn.py:73-106 with one key / value token per batch item, in the dtype of its inputs: (o [B,T,C], attn [B,heads,T]).
    q: [q_batch, T, C]; batch item b reads q[b % q_batch]."""
    assert q.shape[0] == q_batch and k.shape[0] % q_batch == 0
    return _gate_expanded(gate_expand(q, k.shape[0]), k, v, heads, scale)


def _gate_expanded(q, k, v, heads, scale):
    """q: [B, T, C], one query block per batch item, so that its gradient is per batch item as the kernel writes dq."""
    B, T, C = q.shape
    hd = C // heads
    s = (q.view(B, T, heads, hd) * k.view(B, 1, heads, hd)).sum(-1) * scale
    g = torch.sigmoid(s)
    return (g.unsqueeze(-1) * v.view(B, 1, heads, hd)).reshape(B, T, C), g.permute(0, 2, 1)


def gate_expand(q, B, mutant=None):
    qb = q.shape[0]
    if mutant == "qbatch":       # q_batch ignored: item b reads the block b // (B / q_batch) instead of b % q_batch
        return q.repeat_interleave(B // qb, 0)
    return q.repeat(B // qb, 1, 1)


def gate_eval(q, k, v, dout, dattn, heads, scale, model=None, mutant=None):
    """{o, attn, dq, dk, dv}; bf16 model: q, k, v, dout are bf16, o and dq are rounded, attn / dk / dv are f32 (attn_gate.hip)."""
    dt, rnd = _arith(model)
    B = k.shape[0]
    T = q.shape[1]
    if mutant == "drop_token":   # the last token row never processed
        r = gate_eval(q[:, :T - 1], k, v, dout[:, :T - 1], None if dattn is None else dattn[..., :T - 1], heads, scale, model)
        pad = lambda t, dim: torch.cat((t, torch.zeros([1 if i == dim else n for i, n in enumerate(t.shape)], dtype=t.dtype)), dim)
        return {"o": pad(r["o"], 1), "attn": pad(r["attn"], 2), "dq": pad(r["dq"], 1), "dk": r["dk"], "dv": r["dv"]}
    qx = rnd(gate_expand(q.to(dt), B, mutant)).clone().requires_grad_(True)
    kr, vr = rnd(k.to(dt)).clone().requires_grad_(True), rnd(v.to(dt)).clone().requires_grad_(True)
    o, attn = _gate_expanded(qx, kr, vr, heads, scale)
    loss = (o * rnd(dout.to(dt))).sum()
    if dattn is not None:
        loss = loss + (attn * dattn.to(dt)).sum()
    loss.backward()
    return {"o": rnd(o.detach()), "attn": attn.detach().contiguous(), "dq": rnd(qx.grad), "dk": kr.grad, "dv": vr.grad}


def gate_inputs(family, heads, hd, T, B, qb, with_dattn, seed):
    """(q [qb,T,C], k, v [B,C], dout [B,T,C], dattn [B,heads,T] or None) f32."""
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    q, k, v, dout = (torch.randn(s, generator=g) for s in ((qb, T, C), (B, C), (B, C), (B, T, C)))
    dattn = torch.randn((B, heads, T), generator=g) if with_dattn else None
    if family == "saturated":
        # heads 0 .. ceil(heads / 2) - 1: scale q . k = +40 (token + head even) or -40.  The items that share a query row
        # share the key of those heads, so one query can saturate them all.
        ns, scale = (heads + 1) // 2, hd ** -0.5
        k = k.view(B, heads, hd).clone()
        k[:, :ns] = k[torch.arange(B) % qb, :ns]
        kq = k[:qb, :ns]                                                    # [qb, ns, hd]
        kn = kq / kq.norm(dim=-1, keepdim=True)
        qh = q.view(qb, T, heads, hd).clone()
        sign = 1.0 - 2.0 * ((torch.arange(T)[:, None] + torch.arange(ns)[None, :]) % 2)      # [T, ns]
        tgt = sign[None] * 40.0 / (scale * kq.norm(dim=-1))[:, None, :]     # [qb, T, ns]: q's component along the key
        along = (qh[:, :, :ns] * kn[:, None]).sum(-1)
        qh[:, :, :ns] = qh[:, :, :ns] + (tgt - along)[..., None] * kn[:, None]
        q, k = qh.reshape(qb, T, C), k.reshape(B, C)
    elif family != "gaussian":
        raise ValueError(family)
    return q.contiguous(), k.contiguous(), v, dout, dattn


GATE_HEADS = ((4, 76), (4, 28), (4, 128), (4, 4), (2, 64), (8, 32), (1, 128), (3, 20))
GATE_T = (1, 3, 5, 37)
GATE_BQ = ((3, 3), (4, 2), (3, 1))


def gate_cases():
    """(id, family, heads, hd, T, B, q_batch, with_dattn, seed): every head layout x every (B, q_batch); T, dattn and the
    family cycle so that every value of every axis appears."""
    out = []
    for i, (heads, hd) in enumerate(GATE_HEADS):
        for j, (B, qb) in enumerate(GATE_BQ):
            n = i * len(GATE_BQ) + j
            fam, T, da = ("gaussian", "saturated")[n % 2], GATE_T[(n + n // 4) % 4], (n // 2) % 2 == 0
            out.append((f"{fam}-{heads}x{hd}-T{T}-B{B}q{qb}-{'dattn' if da else 'nodattn'}", fam, heads, hd, T, B, qb, da, 4000 + n))
    return out


def gate_mutants(B, qb):
    return ["drop_token"] + (["qbatch"] if 1 < qb < B else [])


# ---- one-key collapse -------------------------------------------------------------------------------------------------
def rank1_ref(x, k, v, wq, wp, bp, heads, scale, reps):
    """attn.py:73-106 + the block's residual (attn.py:153-156) as CAVP calls it with one audio token per batch item: q projection,
    per-head sigmoid(scale q k^T), gate times v, output projection (+ bias) + residual; in the dtype of its inputs.
    Returns (out [B,T,C], attn [B,heads,T]); x: [xb, T, C], B = xb * reps."""
    xr = x.repeat(reps, 1, 1)                                     # cavp_model.py:181: torch.cat((fea_v, fea_v.clone()))
    return rank1_ref_expanded(xr, k, v, wq, wp, bp, heads, scale)


def rank1_ref_expanded(xr, k, v, wq, wp, bp, heads, scale):
    b, t, c = xr.shape
    d = c // heads
    q = (xr @ wq.t()).view(b, t, heads, d)
    s = (q * k.view(b, 1, heads, d)).sum(-1) * scale              # [B, T, H]: q @ k^T with ONE key
    g = torch.sigmoid(s)
    o = (g.unsqueeze(-1) * v.view(b, 1, heads, d)).reshape(b, t, c)
    out = xr + o @ wp.t()
    return (out + bp if bp is not None else out), g.permute(0, 2, 1)


def rank1_eval(x, k, v, wq, wp, bp, dout, heads, scale, reps, model=None, mutant=None):
    """{out, attn, dx, dwq, dwp, dbp, dk, dv}; dx sums the repeats.  bf16 model: x, k, v, dout are bf16 (the weights stay f32), out
    is rounded, and dx is rounded after every repeat's contribution - the kernel keeps the running sum in dx itself
    (attn_rank1.hip); every other gradient is f32."""
    dt, rnd = _arith(model)
    xb, T, C = x.shape
    if mutant == "drop_token":
        r = rank1_eval(x[:, :T - 1], k, v, wq, wp, bp, dout[:, :T - 1], heads, scale, reps, model)
        z = lambda t, dim: torch.cat((t, torch.zeros([1 if i == dim else n for i, n in enumerate(t.shape)], dtype=t.dtype)), dim)
        return dict(r, out=z(r["out"], 1), attn=z(r["attn"], 2), dx=z(r["dx"], 1))
    xr = rnd(x.to(dt)).repeat(reps, 1, 1).clone().requires_grad_(True)
    kr, vr = rnd(k.to(dt)).clone().requires_grad_(True), rnd(v.to(dt)).clone().requires_grad_(True)
    wqr, wpr = wq.to(dt).clone().requires_grad_(True), wp.to(dt).clone().requires_grad_(True)
    bpr = bp.to(dt).clone().requires_grad_(True) if bp is not None else None
    out, attn = rank1_ref_expanded(xr, kr, vr, wqr, wpr, bpr, heads, scale)
    d = rnd(dout.to(dt))
    (out * d).sum().backward()
    gx = xr.grad.view(reps, xb, T, C)
    dx = rnd(gx[0])
    if mutant != "no_repsum":     # the repeat sum of dx omitted: only the first repeat's contribution
        for r in range(1, reps):
            dx = rnd(dx + gx[r])
    return {"out": rnd(out.detach()), "attn": attn.detach().contiguous(), "dx": dx, "dwq": wqr.grad, "dwp": wpr.grad,
            "dbp": bpr.grad if bp is not None else d.sum((0, 1)), "dk": kr.grad, "dv": vr.grad}


def rank1_inputs(family, C, T, xb, reps, with_bp, seed):
    """(x [xb,T,C], k, v [B,C], wq, wp [C,C], bp [C] or None, dout [B,T,C]) f32, 4 heads."""
    g = torch.Generator().manual_seed(seed)
    heads, B = 4, xb * reps
    d = C // heads
    x, k, v = (torch.randn(s, generator=g) for s in ((xb, T, C), (B, C), (B, C)))
    wq, wp = torch.randn((C, C), generator=g) * C ** -0.5, torch.randn((C, C), generator=g) * C ** -0.5
    bp = torch.randn(C, generator=g) * 0.1
    dout = torch.randn((B, T, C), generator=g)
    if family == "saturated":
        # heads 0, 1: x . u[b, h] = +40 (token + head even) or -40, u[b, h] = scale Wq[h-slice]^T k[b, h-slice].  The repeats of
        # an x row share the key of those heads; x moves by the least-norm correction that meets both targets.
        scale = d ** -0.5
        k = k.view(B, heads, d).clone()
        k[:, :2] = k[torch.arange(B) % xb, :2]
        U = scale * torch.einsum("hji,bhj->bhi", wq.view(heads, d, C)[:2].double(), k[:xb, :2].double())      # [xb, 2, C]
        sign = 1.0 - 2.0 * ((torch.arange(T)[:, None] + torch.arange(2)[None, :]) % 2)                          # [T, 2]
        need = 40.0 * sign[None].double() - torch.einsum("btc,bhc->bth", x.double(), U)                        # [xb, T, 2]
        gram = torch.einsum("bhc,bgc->bhg", U, U)
        x = (x.double() + torch.einsum("bth,bhc->btc", torch.linalg.solve(gram[:, None], need[..., None])[..., 0], U)).float()
        k = k.reshape(B, C)
    elif family != "gaussian":
        raise ValueError(family)
    return x.contiguous(), k.contiguous(), v, wq, wp, (bp if with_bp else None), dout


def rank1_logits(x, k, wq, heads, scale, reps):
    xr = x.double().repeat(reps, 1, 1)
    b, t, c = xr.shape
    return ((xr @ wq.double().t()).view(b, t, heads, c // heads) * k.double().view(b, 1, heads, c // heads)).sum(-1) * scale


RANK1_C = (8, 16, 112, 304, 512)
RANK1_T = (1, 2, 3, 5, 33)
RANK1_XR = ((1, 1), (3, 3), (8, 2), (2, 1))


def rank1_cases():
    """(id, family, C, T, xb, reps, with_bp, with_dbp, seed): every C x every (xb, reps); T, bp, dbp and the family cycle."""
    out = []
    for i, C in enumerate(RANK1_C):
        for j, (xb, reps) in enumerate(RANK1_XR):
            n = i * len(RANK1_XR) + j
            fam, T, wb, wd = ("gaussian", "saturated")[n % 2], RANK1_T[(n + n // 5) % 5], (n // 2) % 2 == 0, (n // 4 + n) % 2 == 0
            out.append((f"{fam}-C{C}-T{T}-x{xb}r{reps}-{'bp' if wb else 'nobp'}-{'dbp' if wd else 'nodbp'}", fam, C, T, xb, reps, wb, wd,
                        5000 + n))
    return out


def rank1_mutants(reps):
    return ["drop_token"] + (["no_repsum"] if reps > 1 else [])


# ---- bars ---------------------------------------------------------------------------------------------------------------
def round_inputs(tensors, dtype):
    """What a kernel of `dtype` is given, back in f32: the reference and the models start from the same values."""
    return [None if t is None else (t if dtype == F32 else _rb(t)) for t in tensors]


def sra_o_bound(kv, heads):
    """bf16 forward bound per (batch item, head), broadcastable against o [B, Nq, C]: 1.5 * 2 * 2^-9 * Vmax.  P is rounded to bf16
    (2^-9 relative per weight) and normalised by the unrounded sum: |sum_k (P~ - P) v| <= 2^-9 Vmax; the output (|o| <= Vmax) is
    rounded once more: 2^-9 Vmax.  The factor 1.5 covers the f32 accumulation and the hardware exp."""
    B, Nk, C2 = kv.shape
    C = C2 // 2
    vmax = kv[..., C:].reshape(B, Nk, heads, C // heads).abs().amax((1, 3))          # [B, heads]
    return (1.5 * 2.0 * 2.0 ** -9 * vmax.double())[:, None, :, None].expand(B, 1, heads, C // heads).reshape(B, 1, C)


def ratios(got, ref, cal, dtype, o_bound=None, names=None):
    """err / bar per output.  ref: float64 outputs; cal: the outputs of the model of `dtype` ("f32" / "bf16") on the same inputs;
    o_bound: the element-wise bound of the SRA bf16 forward output (replaces the calibrated bar of "o")."""
    out = {}
    for name in (names if names is not None else ref.keys()):
        if name == "o" and o_bound is not None:
            out[name] = float(((got[name].to(F64) - ref[name]).abs() / o_bound).max())
            continue
        err, e = rel_err(got[name], ref[name]), rel_err(cal[name], ref[name])
        bar = max(4.0 * e, 1e-6) if dtype == F32 else 3.0 * e
        out[name] = err / bar if bar > 0.0 else (0.0 if err == 0.0 else math.inf)
    return out


def within(r):
    """every ratio <= 1 (a NaN ratio is a miss)"""
    return all(v <= 1.0 for v in r.values())


# ---- one case = inputs as the kernel of `dtype` sees them, float64 reference, calibration model ------------------------
def _model_of(dtype):
    return "f32" if dtype == F32 else "bf16"


def sra_setup(case, dtype):
    _, fam, B, heads, Nq, Nk, seed = case
    q, kv, dout = round_inputs(sra_inputs(fam, B, heads, Nq, Nk, seed), dtype)
    ref = sra_grads_autograd(q, kv, dout, heads, 0.125)
    cal = sra_eval(q, kv, dout, heads, 0.125, model=_model_of(dtype))
    return (q, kv, dout), ref, cal, (sra_o_bound(kv, heads) if dtype != F32 else None)


def gate_setup(case, dtype):
    _, fam, heads, hd, T, B, qb, da, seed = case
    q, k, v, dout, dattn = gate_inputs(fam, heads, hd, T, B, qb, da, seed)
    q, k, v, dout = round_inputs((q, k, v, dout), dtype)
    scale = hd ** -0.5
    return (q, k, v, dout, dattn), gate_eval(q, k, v, dout, dattn, heads, scale), \
        gate_eval(q, k, v, dout, dattn, heads, scale, model=_model_of(dtype))


def rank1_setup(case, dtype):
    _, fam, C, T, xb, reps, wb, wd, seed = case
    x, k, v, wq, wp, bp, dout = rank1_inputs(fam, C, T, xb, reps, wb, seed)
    x, k, v, dout = round_inputs((x, k, v, dout), dtype)
    scale = (C // 4) ** -0.5
    return (x, k, v, wq, wp, bp, dout), rank1_eval(x, k, v, wq, wp, bp, dout, 4, scale, reps), \
        rank1_eval(x, k, v, wq, wp, bp, dout, 4, scale, reps, model=_model_of(dtype))
