// ResNet-18 audio encoder (audio_network.py:18-25 of the reference, torchvision's resnet18): the two launches that the igemm convs do
// not cover.  cavp_audio_stem_pool = conv1 7x7/2 + folded bn1 + ReLU + 3x3/2 max pool in one launch (the stem map never reaches HBM);
// cavp_global_maxpool_nhwc = AdaptiveMaxPool2d((1, 1)).  The sixteen 3x3 and three 1x1 convs in between go through cavp_conv2d_nhwc.
#include "host_util.h"

// ------------------------------------------------------------------------------------------------------------
// stem: one workgroup per tile of PH x PW pooled pixels x all 64 channels
// ------------------------------------------------------------------------------------------------------------
// A pooled pixel (ph, pw) is the max over stem pixels (2 ph - 1 + dr, 2 pw - 1 + dc), dr, dc in 0..2, and a stem pixel (sr, sc) reads
// input rows 2 sr - 3 .. 2 sr + 3: the tile needs a (2 PH + 1) x (2 PW + 1) stem tile and a (4 PH + 7) x (4 PW + 7) input patch per channel.
// LDS: the weights transposed to [Cin][7][7][64] f32 (staged once per workgroup; the workgroup then walks tiles with a grid stride), the
// input patch (zero outside the image = the conv's padding), and the stem tile in the OUTPUT dtype - rounding is monotone, so the max
// of the rounded values is the rounded max and bf16 halves the tile.
// Compute: a work item is 8 output channels x AS_R consecutive stem columns of one stem row (48 f32 accumulators); per kernel row it
// reads 2 (AS_R - 1) + 7 input samples and 7 x 8 weights (two 16-byte LDS reads each) for 7 x AS_R x 8 FMAs.
// Pool: stem positions outside the stem map are WRITTEN AS 0 into the tile.  Post-ReLU values are >= 0 and every 3x3/2/1 window holds
// at least its centre (2 ph, 2 pw), which is always in range, so this equals skipping them (nn.MaxPool2d's -inf padding).
constexpr int AS_PH = 4, AS_PW = 8;
constexpr int AS_SR = 2 * AS_PH + 1, AS_SC = 2 * AS_PW + 1;      // stem tile 9 x 17
constexpr int AS_R = 6, AS_NS = (AS_SC + AS_R - 1) / AS_R;       // 3 strips of 6 stem columns (one column of the last is unused)
constexpr int AS_IR = 4 * AS_PH + 7;                             // 23 input rows
constexpr int AS_IC = 2 * (AS_NS * AS_R - 1) + 7;                // 41 input columns: what the strips read, >= 4 PW + 7 (odd: no bank pattern)
constexpr int AS_CO = 64;
static_assert(AS_IC >= 4 * AS_PW + 7, "the patch covers the stem tile");

template <int CIN> constexpr int as_patch_floats() { return (CIN * AS_IR * AS_IC + 3) & ~3; }   // keeps the stem tile 16-byte aligned
template <int CIN> constexpr int as_lds_floats() { return CIN * 49 * AS_CO + as_patch_floats<CIN>(); }
template <typename T, int CIN> constexpr size_t as_lds_bytes() {
  return (size_t)as_lds_floats<CIN>() * 4 + (size_t)AS_SR * AS_SC * AS_CO * sizeof(T);
}

template <typename T, int CIN>
__global__ __launch_bounds__(256) void audio_stem_pool_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              T* __restrict__ y, int H, int W, int Hs, int Ws, int Hp, int Wp,
                                                              int tiles_h, int tiles_w, int total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char as_smem[];
  float* wl = (float*)as_smem;                       // [CIN][7][7][64]
  float* patch = wl + CIN * 49 * AS_CO;              // [CIN][AS_IR][AS_IC]
  T* tile = (T*)(patch + as_patch_floats<CIN>());    // [AS_SR][AS_SC][64]
  constexpr int VE = VecT<T>::VE, CV = AS_CO / VE;
  const int tid = threadIdx.x;

  // OIHW -> [tap][o]: lane -> o, so the LDS writes are conflict-free and the global reads gather from 25 KB that stay in cache
  for (int i = tid; i < CIN * 49 * AS_CO; i += 256) {
    const int o = i & (AS_CO - 1), t = i >> 6;
    wl[i] = w[o * (CIN * 49) + t];
  }

  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    const int tw = item % tiles_w, r1 = item / tiles_w, th = r1 % tiles_h, n = r1 / tiles_h;
    const int ph0 = th * AS_PH, pw0 = tw * AS_PW;
    const int sr0 = 2 * ph0 - 1, sc0 = 2 * pw0 - 1;          // stem coordinates of the tile's corner
    const int ir0 = 2 * sr0 - 3, ic0 = 2 * sc0 - 3;          // input coordinates of the patch's corner
    __syncthreads();                                         // the previous tile's pool reads (and, first, the weight writes) are done
    for (int i = tid; i < CIN * AS_IR * AS_IC; i += 256) {
      const int c = i % AS_IC, q = i / AS_IC, r = q % AS_IR, ci = q / AS_IR;
      const int hi = ir0 + r, wi = ic0 + c;
      const bool ok = (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
      patch[i] = ok ? x[(((size_t)n * CIN + ci) * H + hi) * W + wi] : 0.f;
    }
    __syncthreads();

    for (int wi_ = tid; wi_ < 8 * AS_SR * AS_NS; wi_ += 256) {
      const int cg = wi_ & 7, pos = wi_ >> 3;
      const int sr = pos / AS_NS, c0 = (pos - sr * AS_NS) * AS_R;
      float acc[AS_R][8];
#pragma unroll
      for (int r = 0; r < AS_R; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
#pragma unroll 1
        for (int kh = 0; kh < 7; ++kh) {
          const float* prow = patch + (ci * AS_IR + 2 * sr + kh) * AS_IC + 2 * c0;
          float in[2 * (AS_R - 1) + 7];
#pragma unroll
          for (int u = 0; u < 2 * (AS_R - 1) + 7; ++u) in[u] = prow[u];
          const float* wrow = wl + ((ci * 7 + kh) * 7) * AS_CO + cg * 8;
#pragma unroll
          for (int kw = 0; kw < 7; ++kw) {
            const float4 wa = *(const float4*)(wrow + kw * AS_CO), wb = *(const float4*)(wrow + kw * AS_CO + 4);
            const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int r = 0; r < AS_R; ++r)
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[r][j] = fmaf(in[2 * r + kw], wv[j], acc[r][j]);
          }
        }
      }
      float sc8[8], sh8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { sc8[j] = scale[cg * 8 + j]; sh8[j] = shift[cg * 8 + j]; }
      const bool row_ok = (unsigned)(sr0 + sr) < (unsigned)Hs;
#pragma unroll
      for (int r = 0; r < AS_R; ++r) {
        const int sc = c0 + r;
        if (sc < AS_SC) {
          const bool ok = row_ok && (unsigned)(sc0 + sc) < (unsigned)Ws;
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = ok ? fmaxf(acc[r][j] * sc8[j] + sh8[j], 0.f) : 0.f;
          T* tp = tile + (sr * AS_SC + sc) * AS_CO + cg * 8;
#pragma unroll
          for (int j = 0; j < 8; j += VE) VecT<T>::store(tp + j, v + j);
        }
      }
    }
    __syncthreads();

    for (int i = tid; i < AS_PH * AS_PW * CV; i += 256) {
      const int cv = i % CV, pp = i / CV, pw = pp % AS_PW, ph = pp / AS_PW;
      if (ph0 + ph < Hp && pw0 + pw < Wp) {
        float m[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) m[j] = 0.f;             // the tile holds values >= 0 (see above)
#pragma unroll
        for (int dr = 0; dr < 3; ++dr)
#pragma unroll
          for (int dc = 0; dc < 3; ++dc) {
            float v[VE];
            VecT<T>::load(tile + ((2 * ph + dr) * AS_SC + 2 * pw + dc) * AS_CO + cv * VE, v);
#pragma unroll
            for (int j = 0; j < VE; ++j) m[j] = fmaxf(m[j], v[j]);
          }
        VecT<T>::store(y + (((size_t)n * Hp + ph0 + ph) * Wp + pw0 + pw) * AS_CO + cv * VE, m);
      }
    }
  }
}

// f32 stereo needs 71 KiB of dynamic LDS, past the 64 KiB default; once per instantiation
template <typename T, int CIN>
static void audio_stem_allow_lds() {
  static const hipError_t once = hipFuncSetAttribute((const void*)audio_stem_pool_kernel<T, CIN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)as_lds_bytes<T, CIN>());
  (void)once;
}

extern "C" int cavp_audio_stem_pool(int32_t dtype, const float* x_nchw, const float* w_oihw, const float* scale, const float* shift,
                                    void* y_nhwc, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream) {
  if (!x_nchw || !w_oihw || !scale || !shift || !y_nhwc || N <= 0 || H <= 0 || W <= 0) return CAVP_ERR_BAD_ARG;
  if (Cin != 1 && Cin != 2) return CAVP_ERR_UNSUPPORTED;
  if (!dt_ok(dtype)) return CAVP_ERR_UNSUPPORTED;
  if (!al16(y_nhwc)) return CAVP_ERR_ALIGN;
  const int Hs = (H - 1) / 2 + 1, Ws = (W - 1) / 2 + 1;      // 7x7, stride 2, pad 3
  const int Hp = (Hs - 1) / 2 + 1, Wp = (Ws - 1) / 2 + 1;    // 3x3, stride 2, pad 1
  const int tiles_h = (Hp + AS_PH - 1) / AS_PH, tiles_w = (Wp + AS_PW - 1) / AS_PW;
  const long long total = (long long)N * tiles_h * tiles_w;
  if (total > 0x7fffffffll) return CAVP_ERR_UNSUPPORTED;
  // the weights are staged once per workgroup: three workgroups per CU (bf16; two in f32) walk the tiles
  const int nb = (int)(total < 768 ? total : 768);
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
    if (Cin == 1) audio_stem_allow_lds<T, 1>(); else audio_stem_allow_lds<T, 2>();
    if (Cin == 1)
      audio_stem_pool_kernel<T, 1><<<nb, 256, as_lds_bytes<T, 1>(), s>>>(x_nchw, w_oihw, scale, shift, (T*)y_nhwc, H, W, Hs, Ws, Hp, Wp,
                                                                         tiles_h, tiles_w, (int)total);
    else
      audio_stem_pool_kernel<T, 2><<<nb, 256, as_lds_bytes<T, 2>(), s>>>(x_nchw, w_oihw, scale, shift, (T*)y_nhwc, H, W, Hs, Ws, Hp, Wp,
                                                                         tiles_h, tiles_w, (int)total); });
  CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// global max over HW of an NHWC map (row stride ld): grid (channel block, n), four waves stride over the rows (as gap_kernel)
// ------------------------------------------------------------------------------------------------------------
// VEC: a lane owns one 16-byte channel vector (C, ld multiples of VE, 16-byte aligned base); otherwise one channel.  The running maximum
// starts at -inf, never 0: the inputs may be all negative.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gmp_kernel(const T* __restrict__ x, T* __restrict__ y, int HW, int C, int ldx) {
  constexpr int VE = VEC ? VecT<T>::VE : 1;
  __shared__ float part[4][64 * VE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.y, c = (blockIdx.x * 64 + lane) * VE;
  float m[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) m[j] = -INFINITY;
  if (c < C) {
    const T* xp = x + (size_t)n * HW * ldx + c;
    for (int i = wv; i < HW; i += 4) {
      float v[VE];
      if constexpr (VEC) VecT<T>::load(xp + (size_t)i * ldx, v);
      else v[0] = Elem<T>::ld(xp + (size_t)i * ldx);
#pragma unroll
      for (int j = 0; j < VE; ++j) m[j] = fmaxf(m[j], v[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < VE; ++j) part[wv][j * 64 + lane] = m[j];
  __syncthreads();
  if (wv == 0 && c < C) {
#pragma unroll
    for (int j = 0; j < VE; ++j) m[j] = fmaxf(fmaxf(part[0][j * 64 + lane], part[1][j * 64 + lane]), fmaxf(part[2][j * 64 + lane], part[3][j * 64 + lane]));
    T* yp = y + (size_t)n * C + c;
    if constexpr (VEC) VecT<T>::store(yp, m);
    else Elem<T>::st(yp, m[0]);
  }
}

extern "C" int cavp_global_maxpool_nhwc(int32_t dtype, const void* x, void* y, int32_t N, int32_t HW, int32_t C, int32_t ldx,
                                        void* stream) {
  if (!x || !y || N <= 0 || HW <= 0 || C <= 0 || ldx < C) return CAVP_ERR_BAD_ARG;
  if (!dt_ok(dtype)) return CAVP_ERR_UNSUPPORTED;
  if (N > 65535) return CAVP_ERR_UNSUPPORTED;
  const int VE = dt_ve(dtype);
  const bool vec = C % VE == 0 && ldx % VE == 0 && al16(x) && al16(y);
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
    cavp_dispatch_bool(vec, [&](auto v) {
      constexpr bool V = decltype(v)::value;
      const int per = 64 * (V ? (int)VecT<T>::VE : 1);
      gmp_kernel<T, V><<<dim3((C + per - 1) / per, N), 256, 0, s>>>((const T*)x, (T*)y, HW, C, ldx); }); });
  CHECK_LAUNCH();
}
