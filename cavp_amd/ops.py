"""Thin Python wrappers over the C-ABI (include/cavp_hip.h).  torch is used only for device memory and the current
HIP stream; every arithmetic operation is a kernel in libcavp_hip.so.

Tensors are NHWC "views": a torch tensor of shape [N, H, W, C] whose strides are (H*W*ld, W*ld, ld, 1) with
ld >= C — i.e. possibly a channel slice `buf[..., c0:c1]` of a wider buffer (free concat)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_RELU, BF16, F32, ConvDesc  # noqa: F401

_TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16}
_CODE = {torch.float32: F32, torch.bfloat16: BF16}

_workspace = {}
_retired = []   # outgrown workspaces: never freed, because a captured hipGraph may have baked their address in


def torch_dtype(code: int) -> torch.dtype:
    return _TORCH_DTYPE[code]


def dtype_code(t: torch.dtype) -> int:
    try:
        return _CODE[t]
    except KeyError:
        raise _lib.CavpError(f"unsupported dtype {t}: the HIP path computes in float32 or bfloat16") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.CavpError("libcavp_hip kernels need HIP device tensors; got a CPU tensor (there is no CPU fallback)")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nhwc(t: torch.Tensor) -> Tuple[int, int, int, int, int]:
    """(N, H, W, C, ld) of an NHWC view; validates the stride pattern."""
    if t.dim() != 4:
        raise _lib.CavpError(f"expected an NHWC 4-d view, got shape {tuple(t.shape)}")
    n, h, w, c = t.shape
    sn, sh, sw, sc = t.stride()
    # size-1 dims carry arbitrary strides: take ld from the innermost spatial dim that actually strides
    if w > 1:
        ld = sw
    elif h > 1:
        ld = sh
    elif n > 1:
        ld = sn
    else:
        ld = c
    if c > 1 and sc != 1:
        raise _lib.CavpError("NHWC view must be dense along channels")
    if (w > 1 and sw != ld) or (h > 1 and sh != w * ld) or (n > 1 and sn != h * w * ld) or ld < c:
        raise _lib.CavpError(f"not a dense NHWC view: shape {tuple(t.shape)} stride {t.stride()}")
    return n, h, w, c, ld


_ws_slot = [0]


class workspace_slot:
    """Kernels launched on a second stream concurrently with the main one (TrainPass side sections) must not share the split-K /
    weight-gradient slab scratch: inside this context `workspace()` hands out slot `k`'s own buffer."""

    def __init__(self, k: int):
        self.k = k

    def __enter__(self):
        self.prev = _ws_slot[0]
        _ws_slot[0] = self.k

    def __exit__(self, *exc):
        _ws_slot[0] = self.prev
        return False


def workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Grow-only scratch buffer per device (split-K slabs).  Must not grow while a graph is being captured.  A buffer that
    is outgrown later (say validation at another resolution after capture_train_step) is RETIRED, not freed: graphs captured
    earlier keep replaying into the address they recorded, and the caching allocator must never hand that memory to anyone
    else.  Sizes at least double, so the retired buffers sum to less than the live one."""
    if nbytes <= 0:
        return None
    key = (torch.device(device).index or 0, _ws_slot[0])
    ws = _workspace.get(key)
    if ws is None or ws.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.CavpError("workspace would grow during hipGraph capture; run one eager warm-up pass first")
        if ws is not None:
            _retired.append(ws)
        ws = torch.empty(max(nbytes, 64 << 20, 2 * (ws.numel() if ws is not None else 0)), dtype=torch.uint8, device=device)
        _workspace[key] = ws
    return ws


def conv2d(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, kh: int = 1, kw: int = 1, stride: int = 1,
           pad: int = 0, dil: int = 1, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
           nbias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: int = ACT_NONE,
           splitk: int = 0, tile: int = 0, want_tile_stats: bool = False, stride_w: int = 0,
           res_rows: int = 0, aux: Optional[torch.Tensor] = None, aux_mode: int = 0):
    """out = act((conv(x, w) + nbias[n]) * scale + shift + residual); x/out/residual NHWC views, w OHWI packed.
    res_rows > 0: `residual` has res_rows pixel rows and output pixel p adds row p % res_rows (a batch-periodic residual).
    aux / aux_mode: 1 = act is GELU and gelu'(pre-activation) is stored into `aux` (out's shape); 2 = the result is multiplied
    by `aux` before the residual is added (include/cavp_hip.h, cavp_conv_desc.aux_mode).
    want_tile_stats=True (plain convs only) returns (out, stats) where stats is None when this launch cannot produce the
    fused BatchNorm statistics, else (tile_stats f32 [tiles][Cout][2], tiles, rows_per_tile)."""
    _need_gpu(x, w, out, scale, shift, nbias, residual)
    lib = _lib.load()
    n, h, wd, cin, ldx = _nhwc(x)
    no, ho, wo, cout, ldy = _nhwc(out)
    dt = dtype_code(x.dtype)
    if w.dtype != x.dtype or out.dtype != x.dtype:
        raise _lib.CavpError("conv2d: x, w and out must share one dtype")
    if w.numel() != cout * kh * kw * cin or not w.is_contiguous():
        raise _lib.CavpError(f"conv2d: packed weight has {w.numel()} elements, expected {cout}x{kh}x{kw}x{cin}")
    eho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    ewo = (wd + 2 * pad - dil * (kw - 1) - 1) // (stride_w or stride) + 1
    if (no, ho, wo) != (n, eho, ewo):
        raise _lib.CavpError(f"conv2d: out view is {(no, ho, wo)}, expected {(n, eho, ewo)}")
    ldr = 0
    if residual is not None:
        rn, rh, rw, rc, ldr = _nhwc(residual)
        if res_rows:
            if rn * rh * rw != res_rows or rc != cout or residual.dtype != x.dtype or (n * eho * ewo) % res_rows:
                raise _lib.CavpError("conv2d: a periodic residual must have res_rows rows dividing the output's")
        elif (rn, rh, rw, rc) != (n, eho, ewo, cout) or residual.dtype != x.dtype:
            raise _lib.CavpError("conv2d: residual must match the output view")
    ld_aux = 0
    if aux_mode:
        an, ah, aw, ac, ld_aux = _nhwc(aux)
        if (an, ah, aw, ac) != (n, eho, ewo, cout) or aux.dtype != x.dtype:
            raise _lib.CavpError("conv2d: aux must match the output view")
    for name, v in (("scale", scale), ("shift", shift)):
        if v is not None and (v.dtype != torch.float32 or v.numel() != cout or not v.is_contiguous()):
            raise _lib.CavpError(f"conv2d: {name} must be a contiguous f32 [{cout}]")
    if nbias is not None and (nbias.dtype != torch.float32 or nbias.numel() != n * cout or not nbias.is_contiguous()):
        raise _lib.CavpError(f"conv2d: nbias must be a contiguous f32 [{n},{cout}]")
    d = ConvDesc(dtype=dt, N=n, H=h, W=wd, Cin=cin, ldx=ldx, Cout=cout, ldy=ldy, KH=kh, KW=kw, stride=stride, pad=pad,
                 dil=dil, ldr=ldr, act=act, splitk=splitk, tile=tile, up=0, Ho=0, Wo=0, stride_w=stride_w,
                 res_rows=res_rows if residual is not None else 0, aux_mode=aux_mode, ld_aux=ld_aux)
    nbytes = lib.cavp_conv2d_workspace_bytes(C.byref(d))
    ws = workspace(nbytes, x.device)
    stats = None
    if want_tile_stats:
        tiles, rpt = C.c_int32(0), C.c_int32(0)
        if lib.cavp_conv2d_tile_stats_layout(C.byref(d), C.byref(tiles), C.byref(rpt)) and out.data_ptr() % 16 == 0:
            stats = (torch.empty((tiles.value, cout, 2), dtype=torch.float32, device=x.device), tiles.value, rpt.value)
    st = lib.cavp_conv2d_nhwc_aux(C.byref(d), _ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(nbias), _ptr(residual),
                                  _ptr(out), _ptr(aux) if aux_mode else None, _ptr(ws),
                                  C.c_size_t(ws.numel() if ws is not None else 0),
                                  _ptr(stats[0]) if stats is not None else None, C.c_void_p(_stream()))
    _lib.check(st, f"cavp_conv2d_nhwc N{n} H{h} W{wd} Cin{cin} Cout{cout} k{kh}x{kw} s{stride} p{pad} d{dil}")
    if want_tile_stats:
        return out, stats
    return out


def linear(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, scale=None, residual=None,
           nbias=None, act: int = ACT_NONE, splitk: int = 0, tile: int = 0, res_rows: int = 0) -> torch.Tensor:
    """x: [B, T, Cin] (or [B, Cin]) view, out: [B, T, Cout].  Linear = 1x1 conv over N=B, H=1, W=T."""
    def as4(t):
        if t is None:
            return None
        if t.dim() == 2:
            return t.unsqueeze(1).unsqueeze(1)
        if t.dim() == 3:
            return t.unsqueeze(1)
        return t
    conv2d(as4(x), w, as4(out), scale=scale, shift=bias, nbias=nbias, residual=as4(residual), act=act,
           splitk=splitk, tile=tile, res_rows=res_rows)
    return out


def conv3x3_smallcin_nchw(x_nchw: torch.Tensor, w_oihw: torch.Tensor, out: torch.Tensor, *, stride: int, scale=None,
                          shift=None, act: int = ACT_NONE) -> torch.Tensor:
    _need_gpu(x_nchw, w_oihw, out, scale, shift)
    lib = _lib.load()
    if x_nchw.dtype != torch.float32 or w_oihw.dtype != torch.float32 or not x_nchw.is_contiguous() or not w_oihw.is_contiguous():
        raise _lib.CavpError("conv3x3_smallcin_nchw: x and w must be contiguous f32 (NCHW / OIHW)")
    n, cin, h, w = x_nchw.shape
    cout = w_oihw.shape[0]
    no, ho, wo, co, ldy = _nhwc(out)
    if tuple(w_oihw.shape) != (cout, cin, 3, 3) or co != cout or ldy != cout:
        raise _lib.CavpError("conv3x3_smallcin_nchw: shape mismatch")
    if (no, ho, wo) != (n, (h - 1) // stride + 1, (w - 1) // stride + 1):
        raise _lib.CavpError("conv3x3_smallcin_nchw: bad output view")
    st = lib.cavp_conv3x3_smallcin_nchw(dtype_code(out.dtype), _ptr(x_nchw), _ptr(w_oihw), _ptr(scale), _ptr(shift),
                                        _ptr(out), n, cin, h, w, cout, stride, act, C.c_void_p(_stream()))
    _lib.check(st, "cavp_conv3x3_smallcin_nchw")
    return out


def maxpool(x: torch.Tensor, out: torch.Tensor, k: int, stride: int, pad: int,
            argmax: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
            act: int = ACT_NONE) -> torch.Tensor:
    """argmax (optional): uint8 tensor of out's shape receiving the window-relative arg-max (for maxpool_bwd).
    scale / shift (f32 [C], both or neither) + act: the pool runs over act(x * scale + shift) - cavp_maxpool_affine_nhwc."""
    _need_gpu(x, out, scale, shift)
    n, h, w, c, ld = _nhwc(x)
    no, ho, wo, co, ldo = _nhwc(out)
    if ld != c or ldo != co or co != c or out.dtype != x.dtype:
        raise _lib.CavpError("maxpool: dense NHWC tensors of one dtype required")
    if (no, ho, wo) != (n, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1):
        raise _lib.CavpError("maxpool: bad output shape")
    if argmax is not None and (argmax.dtype != torch.uint8 or not argmax.is_contiguous() or argmax.numel() != out.numel()
                               or argmax.device != x.device):
        raise _lib.CavpError("maxpool: argmax must be a dense uint8 tensor of the output's shape")
    if (scale is None) != (shift is None):
        raise _lib.CavpError("maxpool: scale and shift come together")
    if scale is not None:
        if scale.dtype != torch.float32 or shift.dtype != torch.float32 or scale.numel() != c or shift.numel() != c:
            raise _lib.CavpError("maxpool: scale / shift must be f32 [C]")
        st = _lib.load().cavp_maxpool_affine_nhwc(dtype_code(x.dtype), _ptr(x), _ptr(scale), _ptr(shift), act, _ptr(out), _ptr(argmax),
                                                  n, h, w, c, k, stride, pad, C.c_void_p(_stream()))
        _lib.check(st, "cavp_maxpool_affine_nhwc")
        return out
    st = _lib.load().cavp_maxpool_nhwc(dtype_code(x.dtype), _ptr(x), _ptr(out), _ptr(argmax), n, h, w, c, k, stride, pad,
                                       C.c_void_p(_stream()))
    _lib.check(st, "cavp_maxpool_nhwc")
    return out


def global_avgpool(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _need_gpu(x, out)
    n, h, w, c, ld = _nhwc(x)
    if out.dtype != torch.float32 or out.numel() != n * c or not out.is_contiguous():
        raise _lib.CavpError("global_avgpool: out must be contiguous f32 [N, C]")
    st = _lib.load().cavp_global_avgpool_nhwc(dtype_code(x.dtype), _ptr(x), _ptr(out), n, h * w, c, ld,
                                              C.c_void_p(_stream()))
    _lib.check(st, "cavp_global_avgpool_nhwc")
    return out


def global_maxpool(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out [N, C] (x's dtype, contiguous) = max over H x W of the NHWC view x: nn.AdaptiveMaxPool2d((1, 1))."""
    _need_gpu(x, out)
    n, h, w, c, ld = _nhwc(x)
    if out.dtype != x.dtype or tuple(out.shape) != (n, c) or not out.is_contiguous():
        raise _lib.CavpError("global_maxpool: out must be contiguous [N, C] of the input's dtype")
    st = _lib.load().cavp_global_maxpool_nhwc(dtype_code(x.dtype), _ptr(x), _ptr(out), n, h * w, c, ld,
                                              C.c_void_p(_stream()))
    _lib.check(st, "cavp_global_maxpool_nhwc")
    return out


def global_maxpool_arg(x: torch.Tensor, out: torch.Tensor, arg: torch.Tensor) -> torch.Tensor:
    """global_maxpool with its winner: arg int32 [N, C] = the first position h * W + w of the maximum (nn.AdaptiveMaxPool2d's rule)."""
    _need_gpu(x, out, arg)
    n, h, w, c, ld = _nhwc(x)
    if out.dtype != x.dtype or tuple(out.shape) != (n, c) or not out.is_contiguous():
        raise _lib.CavpError("global_maxpool_arg: out must be contiguous [N, C] of the input's dtype")
    if arg.dtype != torch.int32 or tuple(arg.shape) != (n, c) or not arg.is_contiguous():
        raise _lib.CavpError("global_maxpool_arg: arg must be contiguous int32 [N, C]")
    st = _lib.load().cavp_global_maxpool_arg_nhwc(dtype_code(x.dtype), _ptr(x), _ptr(out), _ptr(arg), n, h * w, c, ld,
                                                  C.c_void_p(_stream()))
    _lib.check(st, "cavp_global_maxpool_arg_nhwc")
    return out


def audio_stem_pool(x_nchw: torch.Tensor, w_oihw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                    out: torch.Tensor) -> torch.Tensor:
    """ResNet-18 audio stem in one launch: conv 7x7 / 2 / 3 (no bias) -> * scale + shift (folded BatchNorm) -> ReLU -> max pool 3 / 2 / 1.
    x f32 NCHW [N, Cin <= 2, H, W], w f32 OIHW [64, Cin, 7, 7], out dense NHWC [N, Hp, Wp, 64] (f32 or bf16)."""
    _need_gpu(x_nchw, w_oihw, scale, shift, out)
    if x_nchw.dim() != 4 or x_nchw.dtype != torch.float32 or w_oihw.dtype != torch.float32 or not x_nchw.is_contiguous() \
            or not w_oihw.is_contiguous():
        raise _lib.CavpError("audio_stem_pool: x and w must be contiguous f32 (NCHW / OIHW)")
    n, cin, h, w = x_nchw.shape
    if cin not in (1, 2) or tuple(w_oihw.shape) != (64, cin, 7, 7):
        raise _lib.CavpError(f"audio_stem_pool: 1 or 2 input channels and a [64, Cin, 7, 7] weight; got x {tuple(x_nchw.shape)}, "
                             f"w {tuple(w_oihw.shape)}")
    for name, v in (("scale", scale), ("shift", shift)):
        if v.dtype != torch.float32 or v.numel() != 64 or not v.is_contiguous():
            raise _lib.CavpError(f"audio_stem_pool: {name} must be a contiguous f32 [64]")
    no, ho, wo, co, ldy = _nhwc(out)
    hs, ws = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if (no, ho, wo, co) != (n, (hs - 1) // 2 + 1, (ws - 1) // 2 + 1, 64) or ldy != 64 or not out.is_contiguous():
        raise _lib.CavpError("audio_stem_pool: bad output view")
    st = _lib.load().cavp_audio_stem_pool(dtype_code(out.dtype), _ptr(x_nchw), _ptr(w_oihw), _ptr(scale), _ptr(shift), _ptr(out),
                                          n, cin, h, w, C.c_void_p(_stream()))
    _lib.check(st, "cavp_audio_stem_pool")
    return out


def bilinear(x: torch.Tensor, out: torch.Tensor, align_corners: bool) -> torch.Tensor:
    _need_gpu(x, out)
    n, hi, wi, c, ldx = _nhwc(x)
    no, ho, wo, co, ldy = _nhwc(out)
    if no != n or co != c or out.dtype != x.dtype:
        raise _lib.CavpError("bilinear: batch / channel / dtype mismatch")
    st = _lib.load().cavp_bilinear_nhwc(dtype_code(x.dtype), _ptr(x), _ptr(out), n, hi, wi, c, ldx, ho, wo, ldy,
                                        int(align_corners), C.c_void_p(_stream()))
    _lib.check(st, "cavp_bilinear_nhwc")
    return out


def bilinear_to_nchw(x: torch.Tensor, out_nchw: torch.Tensor, align_corners: bool) -> torch.Tensor:
    _need_gpu(x, out_nchw)
    n, hi, wi, c, ldx = _nhwc(x)
    if out_nchw.dtype != torch.float32 or not out_nchw.is_contiguous() or out_nchw.shape[:2] != (n, c):
        raise _lib.CavpError("bilinear_to_nchw: out must be contiguous f32 [N, C, Ho, Wo]")
    ho, wo = out_nchw.shape[-2:]
    st = _lib.load().cavp_bilinear_nhwc_to_nchw(dtype_code(x.dtype), _ptr(x), _ptr(out_nchw), n, hi, wi, c, ldx, ho, wo,
                                                int(align_corners), C.c_void_p(_stream()))
    _lib.check(st, "cavp_bilinear_nhwc_to_nchw")
    return out_nchw


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, eps: float) -> torch.Tensor:
    """x, out: [..., C] row-dense views (last-dim stride 1, uniform row stride)."""
    _need_gpu(x, gamma, beta, out)
    c = x.shape[-1]
    rows = x.numel() // c
    x2, o2 = x.reshape(rows, c), out.reshape(rows, c)
    if x2.data_ptr() != x.data_ptr() or o2.data_ptr() != out.data_ptr() or x2.stride(1) != 1 or o2.stride(1) != 1:
        raise _lib.CavpError("layernorm: rows must be viewable as [rows, C] without a copy")
    if gamma.dtype != torch.float32 or beta.dtype != torch.float32 or out.dtype != x.dtype:
        raise _lib.CavpError("layernorm: gamma/beta f32, out dtype == x dtype")
    st = _lib.load().cavp_layernorm(dtype_code(x.dtype), _ptr(x2), _ptr(gamma), _ptr(beta), _ptr(o2), rows, c,
                                    x2.stride(0) if rows > 1 else c, o2.stride(0) if rows > 1 else c,
                                    C.c_float(eps), C.c_void_p(_stream()))
    _lib.check(st, "cavp_layernorm")
    return out


def layernorm_residual(x: torch.Tensor, branch: torch.Tensor, row_scale: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                       out_sum: torch.Tensor, out_norm: torch.Tensor, eps: float):
    """out_sum = x + row_scale[group of the row] * branch, out_norm = LayerNorm(out_sum) in one pass; dense [groups * n, C]
    tensors of one dtype, row_scale f32 [groups] (timm drop_path's mask / keep per image)."""
    _need_gpu(x, branch, row_scale, gamma, beta, out_sum, out_norm)
    c = x.shape[-1]
    rows = x.numel() // c
    ts = (x, branch, out_sum, out_norm)
    if not all(t.is_contiguous() and t.shape == x.shape and t.dtype == x.dtype for t in ts) or row_scale.dtype != torch.float32 \
            or not row_scale.is_contiguous() or rows % row_scale.numel() or gamma.dtype != torch.float32 or beta.dtype != torch.float32:
        raise _lib.CavpError("layernorm_residual: dense tensors of one shape / dtype, f32 gamma / beta and an f32 factor per row group")
    st = _lib.load().cavp_layernorm_residual(dtype_code(x.dtype), _ptr(x), _ptr(branch), _ptr(row_scale), rows // row_scale.numel(),
                                             _ptr(gamma), _ptr(beta), _ptr(out_sum), _ptr(out_norm), rows, c, c, c, C.c_float(eps),
                                             C.c_void_p(_stream()))
    _lib.check(st, "cavp_layernorm_residual")
    return out_sum, out_norm


def attn_gate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, attn: torch.Tensor, heads: int,
              scale: float) -> torch.Tensor:
    """q may hold fewer batch items than out / k / v (a divisor): batch item b then reads q[b % q_batch]."""
    _need_gpu(q, k, v, out, attn)
    qb = q.shape[0]
    b, t, c = out.shape
    if q.shape[1:] != out.shape[1:] or b % qb:
        raise _lib.CavpError("attn_gate: q must be [q_batch, T, C] with q_batch dividing the batch")
    for name, ten in (("q", q), ("k", k), ("v", v), ("out", out), ("attn", attn)):
        if not ten.is_contiguous():
            raise _lib.CavpError(f"attn_gate: {name} must be contiguous")
    if k.numel() != b * c or v.numel() != b * c or attn.numel() != b * heads * t:
        raise _lib.CavpError("attn_gate: shape mismatch")
    if attn.dtype != torch.float32 or len({q.dtype, k.dtype, v.dtype, out.dtype}) != 1:
        raise _lib.CavpError("attn_gate: dtype mismatch")
    st = _lib.load().cavp_attn_gate(dtype_code(q.dtype), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(attn), b, t, heads,
                                    c // heads, C.c_float(scale), qb, C.c_void_p(_stream()))
    _lib.check(st, "cavp_attn_gate")
    return out


def attn1_usable(attn_mod) -> bool:
    """The one-key collapse fits this attention module: supported shape AND f32, contiguous q / proj weights (a model cast with
    .bfloat16() / .half() keeps the q GEMM + gate + proj GEMM route instead of failing in attn1_prepare)."""
    wq, wp = attn_mod.q.weight, attn_mod.proj.weight
    return (attn1_supported(attn_mod.q.in_features, attn_mod.num_heads) and wq.dtype == torch.float32 and wp.dtype == torch.float32
            and wq.is_contiguous() and wp.is_contiguous())


def attn1_supported(c: int, heads: int) -> bool:
    """The one-key attention collapse (cavp_attn1_*) covers this shape (4 heads, C <= 512, C % 8 == 0)."""
    return bool(_lib.load().cavp_attn1_supported(int(c), int(heads)))


def attn1_prepare(wq: torch.Tensor, wp: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float):
    """u[b,h,:] = scale Wq[h-slice,:]^T k[b,h-slice], p[b,h,:] = Wp[:,h-slice] v[b,h-slice]: f32 [B, heads, C] each.
    wq, wp: the f32 [C, C] nn.Linear weights of attn.q / attn.proj; k, v: [B, C] in the compute dtype."""
    _need_gpu(wq, wp, k, v)
    b, c = k.shape
    if wq.dtype != torch.float32 or wp.dtype != torch.float32 or tuple(wq.shape) != (c, c) or tuple(wp.shape) != (c, c):
        raise _lib.CavpError("attn1_prepare: wq / wp must be f32 [C, C]")
    if k.dtype != v.dtype or v.shape != k.shape or not (wq.is_contiguous() and wp.is_contiguous() and k.is_contiguous() and v.is_contiguous()):
        raise _lib.CavpError("attn1_prepare: k, v must be contiguous [B, C] of one dtype")
    u = torch.empty((b, heads, c), dtype=torch.float32, device=k.device)
    pm = torch.empty((b, heads, c), dtype=torch.float32, device=k.device)
    st = _lib.load().cavp_attn1_prepare(dtype_code(k.dtype), _ptr(wq), _ptr(wp), _ptr(k), _ptr(v), _ptr(u), _ptr(pm), b, c, heads,
                                        C.c_float(scale), C.c_void_p(_stream()))
    _lib.check(st, "cavp_attn1_prepare")
    return u, pm


def attn1_fwd(x: torch.Tensor, u: torch.Tensor, pm: torch.Tensor, bp: Optional[torch.Tensor], out: torch.Tensor, attn: torch.Tensor):
    """out[b,t,:] = x[b % xb, t, :] + bp + sum_h sigmoid(x . u[b,h]) pm[b,h];  attn[b,h,t] = the gate.  x: [xb, T, C], out: [B, T, C]."""
    _need_gpu(x, u, pm, out, attn)
    xb, t, c = x.shape
    b, heads = u.shape[0], u.shape[1]
    if tuple(out.shape) != (b, t, c) or b % xb or tuple(attn.shape) != (b, heads, t) or attn.dtype != torch.float32 or out.dtype != x.dtype:
        raise _lib.CavpError("attn1_fwd: shape / dtype mismatch")
    for ten in (x, u, pm, out, attn):
        if not ten.is_contiguous():
            raise _lib.CavpError("attn1_fwd: contiguous tensors required")
    st = _lib.load().cavp_attn1_fwd(dtype_code(x.dtype), _ptr(x), _ptr(u), _ptr(pm), _ptr(bp) if bp is not None else None, _ptr(out),
                                    _ptr(attn), b, xb, t, c, heads, C.c_void_p(_stream()))
    _lib.check(st, "cavp_attn1_fwd")
    return out


def bn_fold(gamma, beta, mean, var, eps: float, scale: torch.Tensor, shift: torch.Tensor) -> None:
    _need_gpu(gamma, beta, mean, var, scale, shift)
    for t in (gamma, beta, mean, var, scale, shift):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.CavpError("bn_fold: contiguous f32 tensors required")
    st = _lib.load().cavp_bn_fold(_ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), C.c_float(eps), _ptr(scale),
                                  _ptr(shift), gamma.numel(), C.c_void_p(_stream()))
    _lib.check(st, "cavp_bn_fold")


def pack_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """torch OIHW (or [out, in]) f32 parameter -> OHWI packed tensor of `dtype` on the same device."""
    _need_gpu(w)
    wd = w.detach()
    if wd.dtype != torch.float32 or not wd.is_contiguous():
        raise _lib.CavpError("pack_weight: contiguous f32 parameter required")
    if wd.dim() == 2:
        cout, cin, kh, kw = wd.shape[0], wd.shape[1], 1, 1
    else:
        cout, cin, kh, kw = wd.shape
    out = torch.empty((cout, kh, kw, cin), dtype=dtype, device=w.device)
    st = _lib.load().cavp_pack_weight_ohwi(dtype_code(dtype), _ptr(wd), _ptr(out), cout, cin, kh, kw,
                                           C.c_void_p(_stream()))
    _lib.check(st, "cavp_pack_weight_ohwi")
    return out


def cast(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    _need_gpu(src, dst)
    if not src.is_contiguous() or not dst.is_contiguous() or src.numel() != dst.numel():
        raise _lib.CavpError("cast: contiguous tensors of equal size required")
    st = _lib.load().cavp_cast(dtype_code(src.dtype), _ptr(src), dtype_code(dst.dtype), _ptr(dst), src.numel(),
                               C.c_void_p(_stream()))
    _lib.check(st, "cavp_cast")
    return dst


# ---- PVTv2 -------------------------------------------------------------------------------------------------------
def sra_attention(q: torch.Tensor, kv: torch.Tensor, out: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """q, out: [B, Nq, heads*64]; kv: [B, Nk, 2*heads*64] (k | v); softmax attention per head (pvt.py:102-130)."""
    _need_gpu(q, kv, out)
    b, nq, c = q.shape
    nk = kv.shape[1]
    if not (q.is_contiguous() and kv.is_contiguous() and out.is_contiguous()) or kv.shape[2] != 2 * c or out.shape != q.shape:
        raise _lib.CavpError("sra_attention: contiguous [B,Nq,C] / [B,Nk,2C] tensors required")
    st = _lib.load().cavp_sra_attention(dtype_code(q.dtype), _ptr(q), _ptr(kv), _ptr(out), b, nq, nk, heads, c // heads,
                                        C.c_float(scale), C.c_void_p(_stream()))
    _lib.check(st, f"cavp_sra_attention B{b} Nq{nq} Nk{nk} heads{heads}")
    return out


def pack_dwconv_weight(w: torch.Tensor) -> torch.Tensor:
    wd = w.detach().contiguous()
    c = wd.shape[0]
    out = torch.empty((9, c), dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().cavp_pack_dwconv_weight(_ptr(wd), _ptr(out), c, C.c_void_p(_stream())), "cavp_pack_dwconv_weight")
    return out


def dwconv3x3(x: torch.Tensor, w9c: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, act: int = ACT_NONE,
              aux: Optional[torch.Tensor] = None):
    """aux (out's shape, act must be ACT_GELU): receives gelu'(pre-activation) for the backward (cavp_dwconv3x3_nhwc_aux)."""
    _need_gpu(x, w9c, bias, out, aux)
    n, h, w, c, ld = _nhwc(x)
    if ld != c or not out.is_contiguous() or out.shape != x.shape:
        raise _lib.CavpError("dwconv3x3: dense NHWC tensors required")
    if aux is not None and (not aux.is_contiguous() or aux.shape != out.shape or aux.dtype != out.dtype):
        raise _lib.CavpError("dwconv3x3: aux must be a dense tensor of the output's shape and dtype")
    st = _lib.load().cavp_dwconv3x3_nhwc_aux(dtype_code(x.dtype), _ptr(x), _ptr(w9c), _ptr(bias), _ptr(out), _ptr(aux), n, h, w, c,
                                             act, C.c_void_p(_stream()))
    _lib.check(st, "cavp_dwconv3x3_nhwc")
    return out


def dwconv3x3_bwd_data(dy: torch.Tensor, w9c: torch.Tensor, dx: torch.Tensor):
    """dx of the depth-wise 3x3 conv from the forward's packed [9][C] weights (the taps are read in reverse order)."""
    _need_gpu(dy, w9c, dx)
    n, h, w, c, ld = _nhwc(dy)
    if ld != c or not dx.is_contiguous() or dx.shape != dy.shape or dx.dtype != dy.dtype:
        raise _lib.CavpError("dwconv3x3_bwd_data: dense NHWC tensors required")
    st = _lib.load().cavp_dwconv3x3_bwd_data_nhwc(dtype_code(dy.dtype), _ptr(dy), _ptr(w9c), _ptr(dx), n, h, w, c,
                                                  C.c_void_p(_stream()))
    _lib.check(st, "cavp_dwconv3x3_bwd_data_nhwc")
    return dx


def conv_smallcin_kxk(x_nchw: torch.Tensor, w_oihw: torch.Tensor, bias, out: torch.Tensor, ks: int, stride: int, pad: int):
    _need_gpu(x_nchw, w_oihw, bias, out)
    n, cin, h, w = x_nchw.shape
    cout = w_oihw.shape[0]
    st = _lib.load().cavp_conv_smallcin_kxk_nchw(dtype_code(out.dtype), _ptr(x_nchw.contiguous()), _ptr(w_oihw.contiguous()),
                                                 _ptr(bias), _ptr(out), n, cin, h, w, cout, ks, stride, pad,
                                                 C.c_void_p(_stream()))
    _lib.check(st, "cavp_conv_smallcin_kxk_nchw")
    return out


# ---- validation metrics (cavp_amd/metrics.py) -----------------------------------------------------------------------
_METRIC_CODE = {torch.float32: F32, torch.int64: _lib.I64}


def _metric_code(t: torch.Tensor, what: str) -> int:
    try:
        return _METRIC_CODE[t.dtype]
    except KeyError:
        raise _lib.CavpError(f"{what}: dtype {t.dtype} unsupported (float32 or int64)") from None


def _check_labels(labels: torch.Tensor, shape, what: str) -> None:
    if tuple(labels.shape) != tuple(shape) or not labels.is_contiguous():
        raise _lib.CavpError(f"{what}: dense labels of shape {tuple(shape)} required, got {tuple(labels.shape)}")


def _check_counts(M: torch.Tensor, k: int, what: str) -> None:
    """M holds the (K+1) x K confusion counts the kernels add into."""
    if M.dtype != torch.int64 or not M.is_contiguous() or M.numel() != (k + 1) * k:
        raise _lib.CavpError(f"{what}: M must be a dense int64 tensor of (K+1)*K counts")


def seg_confusion(logits: torch.Tensor, labels: torch.Tensor, num_classes: int, ignore: int, M: torch.Tensor) -> torch.Tensor:
    """M[(K+1) * K] (int64, read as u64 counts) += the confusion counts of argmax_c(logits) against labels (include/cavp_hip.h,
    cavp_seg_confusion_nchw).  logits: dense f32 [N, C, H, W]; labels: dense [N, H, W], int64 or float32 holding integers
    (masks); K = num_classes >= C."""
    _need_gpu(logits, labels, M)
    if logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise _lib.CavpError(f"seg_confusion: dense float32 [N, C, H, W] logits required, got {logits.dtype} {tuple(logits.shape)}")
    n, c, h, w = logits.shape
    _check_labels(labels, (n, h, w), "seg_confusion")
    k = int(num_classes)
    if k < c:
        raise _lib.CavpError(f"seg_confusion: num_classes {k} < logit channels {c}")
    _check_counts(M, k, "seg_confusion")
    st = _lib.load().cavp_seg_confusion_nchw(_ptr(logits), _ptr(labels), _metric_code(labels, "seg_confusion"), n, c, h * w, k,
                                             int(ignore), _ptr(M), C.c_void_p(_stream()))
    _lib.check(st, f"cavp_seg_confusion_nchw N{n} C{c} HW{h * w} K{k}")
    return M


def mask_iou_stats(pred: torch.Tensor, target: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[N, 4] (int64) += per image (sum p*t, sum max(p, t), sum (1-t)(1-p), sum t); pred / target dense [N, H, W] of int64 or
    float32 (float values must be integers: masks)."""
    _need_gpu(pred, target, out)
    if pred.dim() != 3 or pred.shape != target.shape:
        raise _lib.CavpError(f"mask_iou_stats: pred and target must be [N, H, W] of one shape, got {tuple(pred.shape)} / {tuple(target.shape)}")
    if not (pred.is_contiguous() and target.is_contiguous()):
        raise _lib.CavpError("mask_iou_stats: dense tensors required")
    n, h, w = pred.shape
    if out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != 4 * n:
        raise _lib.CavpError("mask_iou_stats: out must be a dense int64 [N, 4] tensor")
    st = _lib.load().cavp_mask_iou_stats(_ptr(pred), _metric_code(pred, "mask_iou_stats"), _ptr(target),
                                         _metric_code(target, "mask_iou_stats"), n, h * w, _ptr(out), C.c_void_p(_stream()))
    _lib.check(st, "cavp_mask_iou_stats")
    return out


def fmeasure_hist(src: torch.Tensor, gt: torch.Tensor, thresholds: torch.Tensor, hist: torch.Tensor, channel: int = 1) -> torch.Tensor:
    """hist[N, 2, pr_num + 1] (int32, read as u32 counts) += per image the histogram of bin(p) = #{i : thresholds[i] <= p} over all
    pixels ([n, 0]) and over gt != 0 ([n, 1]).  src: a probability map f32 [N, H, W] whose H x W planes are dense (the images may
    be strided, as in torch.softmax(logits, 1)[:, 1]), or dense f32 logits [N, C, H, W] whose softmax channel `channel` is p;
    gt: dense [N, H, W] float32 or int64; thresholds: ascending f32 [pr_num]."""
    _need_gpu(src, gt, thresholds, hist)
    if src.dtype != torch.float32 or src.dim() not in (3, 4):
        raise _lib.CavpError(f"fmeasure_hist: float32 [N, H, W] probabilities or [N, C, H, W] logits required, got {tuple(src.shape)}")
    n, h, w = (src.shape[0], src.shape[-2], src.shape[-1])
    c = src.shape[1] if src.dim() == 4 else 0
    if c:
        if not src.is_contiguous():
            raise _lib.CavpError("fmeasure_hist: dense [N, C, H, W] logits required")
        ld = c * h * w
    else:
        if (w > 1 and src.stride(2) != 1) or (h > 1 and src.stride(1) != w):
            raise _lib.CavpError(f"fmeasure_hist: the H x W planes of the probability map must be dense, got stride {src.stride()}")
        ld = src.stride(0) if n > 1 else h * w
        if ld < h * w:
            raise _lib.CavpError(f"fmeasure_hist: overlapping probability planes (stride {src.stride()})")
    if c == 1 or (c and not 0 <= channel < c):
        raise _lib.CavpError(f"fmeasure_hist: logits need C >= 2 and 0 <= channel < C (C={c}, channel={channel})")
    if tuple(gt.shape) != (n, h, w) or not gt.is_contiguous():
        raise _lib.CavpError(f"fmeasure_hist: dense gt of shape {(n, h, w)} required, got {tuple(gt.shape)}")
    pr = thresholds.numel()
    if thresholds.dtype != torch.float32 or not thresholds.is_contiguous() or pr < 1:
        raise _lib.CavpError("fmeasure_hist: dense float32 thresholds required")
    if hist.dtype != torch.int32 or not hist.is_contiguous() or hist.numel() != n * 2 * (pr + 1):
        raise _lib.CavpError("fmeasure_hist: hist must be a dense int32 [N, 2, pr_num + 1] tensor")
    st = _lib.load().cavp_fmeasure_hist(_ptr(src), ld, _ptr(gt), _metric_code(gt, "fmeasure_hist"), _ptr(thresholds), n, c,
                                        int(channel), h * w, pr, _ptr(hist), C.c_void_p(_stream()))
    _lib.check(st, "cavp_fmeasure_hist")
    return hist


def seg_predict(lo: torch.Tensor, out_hw, *, mask: Optional[torch.Tensor] = None, prob: Optional[torch.Tensor] = None,
                channel: int = 1, labels: Optional[torch.Tensor] = None, num_classes: Optional[int] = None, ignore: int = -1,
                M: Optional[torch.Tensor] = None, align_corners: bool = False):
    """Class mask, probability map and confusion counts of the bilinearly upsampled logits, from the low-resolution logits `lo`
    (NHWC view [N, h, w, C], f32 or bf16) in one launch; the [N, C, H, W] tensor bilinear_to_nchw would write is never made, yet
    the results are those of its output, bit for bit (include/cavp_hip.h, cavp_seg_predict_nhwc).  Each output is optional, at
    least one is required:
      mask   dense uint8 [N, H, W]  <- argmax over C (C <= 256);
      prob   dense f32 [N, H, W]    <- softmax over C, channel `channel`;
      M      dense int64 (K+1)*K    += confusion counts against `labels` (dense [N, H, W], int64 or float32 holding integers),
             K = num_classes >= C, bin rule of seg_confusion.
    Returns (mask, prob, M)."""
    _need_gpu(lo, mask, prob, labels, M)
    n, hi, wi, c, ldx = _nhwc(lo)
    ho, wo = (int(v) for v in out_hw)
    if mask is None and prob is None and M is None:
        raise _lib.CavpError("seg_predict: ask for at least one of mask, prob, M")
    if ho <= 0 or wo <= 0:
        raise _lib.CavpError(f"seg_predict: bad output size {(ho, wo)}")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_contiguous() or tuple(mask.shape) != (n, ho, wo)):
        raise _lib.CavpError(f"seg_predict: mask must be a dense uint8 {(n, ho, wo)} tensor")
    if mask is not None and c > 256:
        raise _lib.CavpError(f"seg_predict: a uint8 mask holds at most 256 classes, the logits have {c}")
    if prob is not None:
        if prob.dtype != torch.float32 or not prob.is_contiguous() or tuple(prob.shape) != (n, ho, wo):
            raise _lib.CavpError(f"seg_predict: prob must be a dense float32 {(n, ho, wo)} tensor")
        if not 0 <= int(channel) < c:
            raise _lib.CavpError(f"seg_predict: channel {channel} outside the {c} logit channels")
    if (labels is None) != (M is None):
        raise _lib.CavpError("seg_predict: labels and M come together")
    k, code = 0, F32
    if M is not None:
        if num_classes is None:
            raise _lib.CavpError("seg_predict: num_classes is required with M")
        k = int(num_classes)
        _check_labels(labels, (n, ho, wo), "seg_predict")
        if k < c:
            raise _lib.CavpError(f"seg_predict: num_classes {k} < logit channels {c}")
        _check_counts(M, k, "seg_predict")
        code = _metric_code(labels, "seg_predict")
    st = _lib.load().cavp_seg_predict_nhwc(dtype_code(lo.dtype), _ptr(lo), n, hi, wi, c, ldx, ho, wo, int(align_corners), _ptr(mask),
                                           _ptr(prob), int(channel), _ptr(labels), code, k, int(ignore), _ptr(M),
                                           C.c_void_p(_stream()))
    _lib.check(st, f"cavp_seg_predict_nhwc N{n} {hi}x{wi}->{ho}x{wo} C{c} K{k}")
    return mask, prob, M


def clipval_update(pred: torch.Tensor, is_mask: bool, labels: torch.Tensor, count: Optional[torch.Tensor], B: int, T: int, c: int, hw: int,
                   k: int, ignore: int, min_count: int, min_values: int, hist: torch.Tensor, conf: torch.Tensor, flags: torch.Tensor,
                   counts: torch.Tensor, frames: torch.Tensor, state: torch.Tensor) -> None:
    """One ClipValidation update of inputs that metrics.ClipValidation has checked (include/cavp_hip.h, cavp_clipval_frame_counts
    and cavp_clipval_combine): the frames' label histograms and confusion counts into the scratch hist / conf, then the flags
    and the adds into counts [2, K+1, K], frames [2] and state [4]."""
    lib, st = _lib.load(), C.c_void_p(_stream())
    i64 = 1 if count is not None and count.dtype == torch.int64 else 0
    _lib.check(lib.cavp_clipval_frame_counts(_ptr(pred), 1 if is_mask else 0, _ptr(labels), _ptr(count), i64, B, T, c, hw, k, ignore,
                                             _ptr(hist), _ptr(conf), _ptr(state), st),
               f"cavp_clipval_frame_counts B{B} T{T} C{c} HW{hw} K{k}")
    _lib.check(lib.cavp_clipval_combine(_ptr(hist), _ptr(conf), _ptr(flags), _ptr(count), i64, B, T, k, min_count, min_values,
                                        _ptr(counts), _ptr(frames), _ptr(state), st), f"cavp_clipval_combine B{B} T{T} K{k}")


SEMVAL_STATE_WORDS = 4             # {mask bytes >= K, bad counts, frames, ticket}


def semval_update(pred: torch.Tensor, is_mask: bool, labels: torch.Tensor, count: Optional[torch.Tensor], B: int, T: int, c: int, hw: int,
                  k: int, max_frames: int, scratch: torch.Tensor, acc: torch.Tensor, last: torch.Tensor, state: torch.Tensor,
                  combine: bool = True) -> None:
    """One SemanticValidation update of inputs that metrics.SemanticValidation has checked (include/cavp_hip.h,
    cavp_semval_frame_counts and cavp_semval_combine): the frames' class areas and binary sums into the scratch [max_frames, 3K + 4],
    then the float32 tail into acc [3K + 1], last [3K + 1 + 2 * max_frames] and state [4].  combine=False stops after the first
    launch and leaves the integer counts in the scratch (the tests read them there, from a scratch of their own)."""
    E = _lib.CavpError
    if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() != max_frames * (3 * k + 4):
        raise E("semval_update: scratch must be a dense int32 [max_frames, 3K + 4] tensor")
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() != 3 * k + 1:
        raise E("semval_update: acc must be a dense float32 [3K + 1] tensor")
    if last.dtype != torch.float32 or not last.is_contiguous() or last.numel() != 3 * k + 1 + 2 * max_frames:
        raise E("semval_update: last must be a dense float32 [3K + 1 + 2 * max_frames] tensor")
    if state.dtype != torch.int64 or not state.is_contiguous() or state.numel() != SEMVAL_STATE_WORDS:
        raise E(f"semval_update: state must be a dense int64 [{SEMVAL_STATE_WORDS}] tensor")
    if B * T > max_frames:
        raise E(f"semval_update: {B * T} frames, max_frames = {max_frames}")
    _need_gpu(pred, labels, count, scratch, acc, last, state)
    lib, st = _lib.load(), C.c_void_p(_stream())
    i64 = 1 if count is not None and count.dtype == torch.int64 else 0
    _lib.check(lib.cavp_semval_frame_counts(_ptr(pred), 1 if is_mask else 0, _ptr(labels), _ptr(count), i64, B, T, c, hw, k,
                                            _ptr(scratch), _ptr(state), st), f"cavp_semval_frame_counts B{B} T{T} C{c} HW{hw} K{k}")
    if combine:
        _lib.check(lib.cavp_semval_combine(_ptr(scratch), _ptr(count), i64, B, T, hw, k, max_frames, _ptr(acc), _ptr(last),
                                           _ptr(state), st), f"cavp_semval_combine B{B} T{T} K{k}")


VIDEOVAL_MAX_THRESHOLDS = 1024     # CAVP_VIDEOVAL_MAX_THRESHOLDS
VIDEOVAL_STATE_WORDS = 8           # {labels outside {0, 1, ignore}, mask bytes >= K, bad counts, videos dropped, videos seen, ticket, -, -}


def _videoval_scratch(stats: torch.Tensor, hist: torch.Tensor, state: torch.Tensor, n: int, pr: int, what: str) -> None:
    if not 1 <= pr <= VIDEOVAL_MAX_THRESHOLDS:
        raise _lib.CavpError(f"{what}: 1 <= pr_num <= {VIDEOVAL_MAX_THRESHOLDS}, got {pr}")
    if stats.dtype != torch.int64 or not stats.is_contiguous() or stats.numel() < 4 * n:
        raise _lib.CavpError(f"{what}: stats must be a dense int64 tensor of at least [{n}, 4]")
    if hist.dtype != torch.int32 or not hist.is_contiguous() or hist.numel() < n * 2 * (pr + 1):
        raise _lib.CavpError(f"{what}: hist must be a dense int32 tensor of at least [{n}, 2, {pr + 1}]")
    if state.dtype != torch.int64 or not state.is_contiguous() or state.numel() != VIDEOVAL_STATE_WORDS:
        raise _lib.CavpError(f"{what}: state must be a dense int64 [{VIDEOVAL_STATE_WORDS}] tensor")


def _videoval_count(count: Optional[torch.Tensor], n: int, T: int, what: str) -> Tuple[int, int]:
    """(B, count_i64) of N = B * T frames and the optional count [B]."""
    T = int(T)
    if T < 1 or n < 1 or n % T:
        raise _lib.CavpError(f"{what}: {n} frames are no whole number of videos of T = {T}")
    B = n // T
    if n > 65535:
        raise _lib.CavpError(f"{what}: at most 65535 frames in one call, got {n}")
    if count is not None:
        if not isinstance(count, torch.Tensor) or count.dtype not in (torch.int32, torch.int64) or tuple(count.shape) != (B,) \
                or not count.is_contiguous():
            raise _lib.CavpError(f"{what}: count must be a dense int32 or int64 tensor of shape ({B},)")
    return B, 1 if count is not None and count.dtype == torch.int64 else 0


def videoval_frame_stats(pred: torch.Tensor, labels: torch.Tensor, count: Optional[torch.Tensor], T: int, num_classes: int, ignore: int,
                         thresholds: torch.Tensor, stats: torch.Tensor, hist: torch.Tensor, M: torch.Tensor, state: torch.Tensor,
                         channel: int = 1, prob: Optional[torch.Tensor] = None) -> None:
    """One pass over the prediction of N = B * T frames (include/cavp_hip.h, cavp_videoval_frame_stats): per frame n that takes part
    (t < clamp(count[b], 0, T); count None: all) stats[n, 4] (int64) += the sums of mask_iou_stats, hist[n, 2, pr_num + 1] (int32) +=
    the histograms of fmeasure_hist, and M[(K+1) * K] (int64) += the counts of seg_confusion.  pred: dense f32 logits [N, C, H, W]
    with 2 <= C <= K, or a dense uint8 class mask [N, H, W] together with prob, a dense f32 [N, H, W] plane (seg_predict's
    outputs).  labels: dense int64 with N * H * W elements ending in [H, W]; thresholds: ascending f32 [pr_num]; state: int64 [8]."""
    E = _lib.CavpError
    if not isinstance(pred, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise E("videoval_frame_stats: pred and labels are tensors")
    is_mask = pred.dtype == torch.uint8
    k = int(num_classes)
    if is_mask:
        if pred.dim() != 3 or not pred.is_contiguous():
            raise E(f"videoval_frame_stats: a dense uint8 class mask [N, H, W] required, got {tuple(pred.shape)}")
        if prob is None or prob.dtype != torch.float32 or tuple(prob.shape) != tuple(pred.shape) or not prob.is_contiguous():
            raise E(f"videoval_frame_stats: a mask comes with a dense float32 probability plane of its shape {tuple(pred.shape)}")
        c = 0
    elif pred.dtype == torch.float32:
        if pred.dim() != 4 or not pred.is_contiguous():
            raise E(f"videoval_frame_stats: dense float32 logits [N, C, H, W] required, got {tuple(pred.shape)}")
        c = pred.shape[1]
        if c < 2 or not 0 <= int(channel) < c:
            raise E(f"videoval_frame_stats: logits need C >= 2 and 0 <= channel < C (C={c}, channel={channel})")
        if k < c:
            raise E(f"videoval_frame_stats: num_classes {k} < logit channels {c}")
        if prob is not None:
            raise E("videoval_frame_stats: prob comes with a uint8 mask only")
    else:
        raise E(f"videoval_frame_stats: pred is a uint8 class mask [N, H, W] or float32 logits [N, C, H, W], got {pred.dtype}")
    n, h, w = pred.shape[0], pred.shape[-2], pred.shape[-1]
    if n < 1 or h < 1 or w < 1:
        raise E("videoval_frame_stats: empty inputs are not supported")
    if labels.dtype != torch.int64 or labels.dim() < 3 or labels.numel() != n * h * w or tuple(labels.shape[-2:]) != (h, w) \
            or not labels.is_contiguous():
        raise E(f"videoval_frame_stats: dense int64 labels of {n} frames of {(h, w)} required, got {labels.dtype} {tuple(labels.shape)}")
    B, i64 = _videoval_count(count, n, T, "videoval_frame_stats")
    pr = thresholds.numel()
    if thresholds.dtype != torch.float32 or not thresholds.is_contiguous():
        raise E("videoval_frame_stats: dense float32 thresholds required")
    _videoval_scratch(stats, hist, state, n, pr, "videoval_frame_stats")
    _check_counts(M, k, "videoval_frame_stats")
    _need_gpu(pred, prob, labels, count, thresholds, stats, hist, M, state)
    st = _lib.load().cavp_videoval_frame_stats(_ptr(pred), 1 if is_mask else 0, _ptr(prob), _ptr(labels), _ptr(count), i64, B, int(T), c,
                                               int(channel), h * w, k, int(ignore), _ptr(thresholds), pr, _ptr(stats), _ptr(hist),
                                               _ptr(M), _ptr(state), C.c_void_p(_stream()))
    _lib.check(st, f"cavp_videoval_frame_stats B{B} T{T} C{c} HW{h * w} K{k}")


def videoval_combine(stats: torch.Tensor, hist: torch.Tensor, count: Optional[torch.Tensor], B: int, T: int, hw: int, pr_num: int,
                     J: torch.Tensor, F: torch.Tensor, state: torch.Tensor) -> None:
    """The float32 tail of videoval_frame_stats' scratch (include/cavp_hip.h, cavp_videoval_combine): J and F (dense f32 [max_videos])
    of every video with frames into the next free slots, state[4] advanced on the device, the scratch written back to zero."""
    E = _lib.CavpError
    B, T, hw, pr = int(B), int(T), int(hw), int(pr_num)
    if B < 1 or hw < 1:
        raise E("videoval_combine: B >= 1 and HW >= 1")
    _videoval_count(count, B * T, T, "videoval_combine")
    _videoval_scratch(stats, hist, state, B * T, pr, "videoval_combine")
    if J.dtype != torch.float32 or F.dtype != torch.float32 or not (J.is_contiguous() and F.is_contiguous()) or J.dim() != 1 \
            or J.shape != F.shape or J.numel() < 1:
        raise E("videoval_combine: J and F must be dense float32 [max_videos] tensors of one size")
    _need_gpu(stats, hist, count, J, F, state)
    i64 = 1 if count is not None and count.dtype == torch.int64 else 0
    st = _lib.load().cavp_videoval_combine(_ptr(stats), _ptr(hist), _ptr(count), i64, B, T, hw, pr, J.numel(), _ptr(J), _ptr(F),
                                           _ptr(state), C.c_void_p(_stream()))
    _lib.check(st, f"cavp_videoval_combine B{B} T{T} HW{hw}")
