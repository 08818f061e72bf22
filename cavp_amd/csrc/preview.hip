// Preview panels on the device (include/cavp_hip.h, "preview stage"): the three pictures per frame that the reference's
// Tensorboard.upload_wandb_image (utils/tensor_board.py:90-139) makes on the host from whole-tensor copies - the de-normalised
// frame `x`, the label `y` and the prediction `y_tilde` as palette indices - as one streaming launch that reads the logits exactly
// once, plus an optional byte gather for the reference's resize=True.  Indices only: the palette is applied on the host.
//
//   panels: one thread = 4 consecutive pixels ("quad", the pattern of metrics.hip).  16-byte loads per channel plane and whole
//           dword stores (three for x, one each for y and y_tilde) when HW % 4 == 0 and every base is aligned; an element path
//           otherwise (a second image that starts unaligned included).  Vector stores only; the one atomic is the bad counter.
//   resize: a byte gather of the panels through two index tables (PIL's NEAREST rule, made once on the host).
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;

struct NoLabel {};   // labels == NULL: no y panel, no ignore propagation

// torch.argmax: first maximal index, a NaN counts as the maximum (the rule of metrics.hip)
__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& idx) {
  if (v > best || (v != v && best == best)) { best = v; idx = c; }
}

// DeNormalize (t.mul_(s).add_(m)) then ToPILImage (pic.mul(255).byte()): three separately rounded float32 operations, never
// contracted; the byte is the value truncated toward zero, mod 256 (torch's CPU cast).  A non-finite u or |u| >= 2^31: 0, counted.
__device__ __forceinline__ unsigned denorm_byte(float t, float s, float m, unsigned& bad) {
#pragma clang fp contract(off)
  const float v = __fadd_rn(__fmul_rn(t, s), m);
  const float u = __fmul_rn(v, 255.0f);
  if (!(fabsf(u) < 2147483648.0f)) { ++bad; return 0u; }
  return (unsigned)(int)u & 255u;
}

template <typename T, bool kVec>
__device__ __forceinline__ void load4(const T* p, int np, T t[4]) {
  if constexpr (!kVec) {
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = j < np ? p[j] : (T)0;
  } else if constexpr (sizeof(T) == 8) {
    const longlong2 a = *(const longlong2*)p, b = *(const longlong2*)(p + 2);
    t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y;
  } else if constexpr (sizeof(T) == 4) {
    const float4 a = *(const float4*)p;
    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
  } else {
    const unsigned w = *(const unsigned*)p;
    t[0] = w & 255u; t[1] = (w >> 8) & 255u; t[2] = (w >> 16) & 255u; t[3] = w >> 24;
  }
}

// the bytes b[0..3] as one dword (kVec) or the first np of them one by one
template <bool kVec>
__device__ __forceinline__ void store4(unsigned char* p, int np, const unsigned b[4]) {
  if constexpr (kVec) {
    *(unsigned*)p = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < np) p[j] = (unsigned char)b[j];
  }
}

// the logits are read once and never again: their 16-byte loads are non-temporal (a one-off measurement on scratch builds,
// profiles/preview_load_variants.txt: 117.5 -> 109.5 us at B = 32, C = 71, 224 x 224 with 8 plane loads in flight, 111.8 -> 105.8 us with 16)
template <bool kVec>
__device__ __forceinline__ void load4_once(const float* p, int np, float t[4]) {
  if constexpr (kVec) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 a = __builtin_nontemporal_load((const f32x4*)p);
    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
  } else {
    load4<float, false>(p, np, t);
  }
}

// idx[j] = argmax over the C planes (HW apart) of pixel j of the quad at src; every plane is loaded once, 16 loads in flight
template <bool kVec>
__device__ __forceinline__ void quad_argmax(const float* src, int C, long long HW, int np, unsigned idx[4]) {
  int id[4] = {0, 0, 0, 0};
  float best[4];
  load4_once<kVec>(src, np, best);
#pragma unroll 16
  for (int c = 1; c < C; ++c) {
    float v[4];
    load4_once<kVec>(src + c * HW, np, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) argmax_step(v[j], c, best[j], id[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = (unsigned)id[j];
}

// kMask: pred is the u8 class mask [B][HW], else the f32 logits [B][C][HW].  LT: long long, unsigned char or NoLabel.
// image / x may be NULL (no x panel).  Per image the outputs lie `stride` bytes apart.
template <bool kMask, typename LT, bool kVec>
__global__ __launch_bounds__(kThreads) void preview_panels_kernel(const float* __restrict__ image, const float* __restrict__ mean_std,
                                                                  const LT* __restrict__ labels, const void* __restrict__ pred,
                                                                  int B, int C, long long HW, long long ignore,
                                                                  unsigned char* __restrict__ x, unsigned char* __restrict__ y,
                                                                  unsigned char* __restrict__ yt, long long stride,
                                                                  unsigned long long* __restrict__ state) {
  constexpr bool kLab = !std::is_same<LT, NoLabel>::value;
  const long long nq = (HW + 3) >> 2, total = (long long)B * nq;
  float ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (image) {
#pragma unroll
    for (int i = 0; i < 6; ++i) ms[i] = mean_std[i];
  }
  unsigned bad = 0u;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < total; q += (long long)gridDim.x * kThreads) {
    const long long n = q / nq, p0 = (q - n * nq) * 4;
    const int np = kVec ? 4 : (int)(HW - p0 < 4 ? HW - p0 : 4);
    const long long ob = n * stride;
    unsigned p[4];
    if constexpr (kMask) {
      unsigned char m[4];
      load4<unsigned char, kVec>((const unsigned char*)pred + n * HW + p0, np, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = m[j];
    } else {
      quad_argmax<kVec>((const float*)pred + n * C * HW + p0, C, HW, np, p);
    }
    if constexpr (kLab) {
      LT t[4];
      load4<LT, kVec>(labels + n * HW + p0, np, t);
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long v = (long long)t[j];
        w[j] = (unsigned)((unsigned long long)v & 255ull);      // mask.astype(uint8): the wrap mod 256
        if (v == ignore) p[j] = 255u;                             // compared before the wrap
      }
      store4<kVec>(y + ob + p0, np, w);
    }
    store4<kVec>(yt + ob + p0, np, p);
    if (image) {
      unsigned px[12];   // r0 g0 b0 r1 g1 b1 ...
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t[4];
        load4<float, kVec>(image + (n * 3 + c) * HW + p0, np, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j * 3 + c] = j < np ? denorm_byte(t[j], ms[3 + c], ms[c], bad) : 0u;
      }
      unsigned char* xo = x + ob + p0 * 3;
      if constexpr (kVec) {
#pragma unroll
        for (int k = 0; k < 3; ++k) store4<true>(xo + 4 * k, 4, px + 4 * k);
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (k < 3 * np) xo[k] = (unsigned char)px[k];
      }
    }
  }
  if (bad) atomicAdd(state, (unsigned long long)bad);
}

// dst panels [Ho][Wo] from src panels [H][W] of the same per-image layout (x: 3 bytes per pixel when has_x, then y when has_y,
// then y_tilde); one thread = 4 consecutive output pixels of a row; kVec: Wo % 4 == 0 and dst 4-byte aligned (whole dwords)
template <bool kVec>
__global__ __launch_bounds__(kThreads) void preview_resize_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                  const int* __restrict__ row_tab, const int* __restrict__ col_tab,
                                                                  int B, int H, int W, int Ho, int Wo, int has_x, int has_y) {
  const long long HW = (long long)H * W, HWo = (long long)Ho * Wo;
  const int planes = (has_x ? 3 : 0) + (has_y ? 1 : 0) + 1;
  const long long nqw = (Wo + 3) >> 2, total = (long long)B * Ho * nqw;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < total; q += (long long)gridDim.x * kThreads) {
    const long long n = q / (Ho * nqw), r = q - n * (Ho * nqw);
    const int oy = (int)(r / nqw), ox = (int)(r - (long long)oy * nqw) * 4;
    const int np = kVec ? 4 : (Wo - ox < 4 ? Wo - ox : 4);
    const long long srow = (long long)row_tab[oy] * W, drow = (long long)oy * Wo + ox;
    int sx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sx[j] = col_tab[j < np ? ox + j : ox];
    const unsigned char* s = src + n * planes * HW;
    unsigned char* d = dst + n * planes * HWo;
    if (has_x) {
      unsigned px[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned char* sp = s + (srow + sx[j]) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j * 3 + c] = sp[c];
      }
      unsigned char* xo = d + drow * 3;
      if constexpr (kVec) {
#pragma unroll
        for (int k = 0; k < 3; ++k) store4<true>(xo + 4 * k, 4, px + 4 * k);
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (k < 3 * np) xo[k] = (unsigned char)px[k];
      }
      s += 3 * HW;
      d += 3 * HWo;
    }
    for (int pl = has_y ? 0 : 1; pl < 2; ++pl) {
      unsigned b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = s[srow + sx[j]];
      store4<kVec>(d + drow, np, b);
      s += HW;
      d += HWo;
    }
  }
}

inline unsigned grid_for(long long threads) {
  const long long nb = (threads + kThreads - 1) / kThreads;
  return (unsigned)(nb < 1 ? 1 : nb > kMaxBlocks ? kMaxBlocks : nb);
}

inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

template <bool kMask, typename LT>
void panels_launch(bool vec, unsigned grid, hipStream_t s, const float* image, const float* mean_std, const void* labels, const void* pred,
                   int B, int C, long long HW, long long ignore, unsigned char* x, unsigned char* y, unsigned char* yt, long long stride,
                   unsigned long long* state) {
  cavp_dispatch_bool(vec, [&](auto v) {
    preview_panels_kernel<kMask, LT, decltype(v)::value><<<grid, kThreads, 0, s>>>(image, mean_std, (const LT*)labels, pred, B, C, HW,
                                                                                 ignore, x, y, yt, stride, state);
  });
}

}  // namespace

extern "C" int cavp_preview_panels(const float* image, const float* mean_std, const void* labels, int32_t label_u8, const void* pred,
                                   int32_t pred_is_mask, int32_t B, int32_t C, int64_t HW, int64_t ignore, uint8_t* x, uint8_t* y,
                                   uint8_t* y_tilde, int64_t out_stride, int64_t* state, void* stream) {
  if (!pred || !y_tilde || !state || B < 1 || HW < 1 || (!pred_is_mask && C < 1)) return CAVP_ERR_BAD_ARG;
  if ((image != nullptr) != (x != nullptr) || (image && !mean_std) || (labels != nullptr) != (y != nullptr)) return CAVP_ERR_BAD_ARG;
  if (out_stride < ((image ? 3 : 0) + (labels ? 1 : 0) + 1) * HW) return CAVP_ERR_BAD_ARG;
  if (!pred_is_mask && C > 256) return CAVP_ERR_UNSUPPORTED;
  bool vec = HW % 4 == 0 && out_stride % 4 == 0 && al4(y_tilde) && (pred_is_mask ? al4(pred) : al16(pred));
  if (image) vec = vec && al16(image) && al4(x);
  if (labels) vec = vec && al4(y) && (label_u8 ? al4(labels) : al16(labels));
  const unsigned grid = grid_for((long long)B * ((HW + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  auto go = [&](auto mask_tag) {
    constexpr bool kMask = decltype(mask_tag)::value;
    if (!labels)
      panels_launch<kMask, NoLabel>(vec, grid, s, image, mean_std, labels, pred, B, C, HW, ignore, x, y, y_tilde, out_stride,
                                    (unsigned long long*)state);
    else if (label_u8)
      panels_launch<kMask, unsigned char>(vec, grid, s, image, mean_std, labels, pred, B, C, HW, ignore, x, y, y_tilde, out_stride,
                                          (unsigned long long*)state);
    else
      panels_launch<kMask, long long>(vec, grid, s, image, mean_std, labels, pred, B, C, HW, ignore, x, y, y_tilde, out_stride,
                                      (unsigned long long*)state);
  };
  cavp_dispatch_bool(pred_is_mask != 0, go);
  CHECK_LAUNCH();
}

extern "C" int cavp_preview_resize(const uint8_t* src, uint8_t* dst, const int32_t* row_tab, const int32_t* col_tab, int32_t B, int32_t H,
                                   int32_t W, int32_t Ho, int32_t Wo, int32_t has_x, int32_t has_y, void* stream) {
  if (!src || !dst || !row_tab || !col_tab || B < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return CAVP_ERR_BAD_ARG;
  const bool vec = Wo % 4 == 0 && al4(dst);
  const unsigned grid = grid_for((long long)B * Ho * ((Wo + 3) / 4));
  cavp_dispatch_bool(vec, [&](auto v) {
    preview_resize_kernel<decltype(v)::value><<<grid, kThreads, 0, (hipStream_t)stream>>>(src, dst, row_tab, col_tab, B, H, W, Ho, Wo,
                                                                                         has_x ? 1 : 0, has_y ? 1 : 0);
  });
  CHECK_LAUNCH();
}
