// ResNet-18 audio encoder (audio_network.py:18-25 of the reference, torchvision's resnet18): the launches that the igemm convs do
// not cover.  Eval: cavp_audio_stem_pool = conv1 7x7/2 + folded bn1 + ReLU + 3x3/2 max pool in one launch (the stem map never reaches
// HBM); cavp_global_maxpool_nhwc = AdaptiveMaxPool2d((1, 1)).  Training: cavp_audio_stem_train = conv1 raw + the BatchNorm tile statistics
// of its output; cavp_global_maxpool_arg_nhwc / cavp_global_maxpool_bwd_nhwc = the global max with its winner and the backward through
// it.  The sixteen 3x3 and three 1x1 convs in between go through cavp_conv2d_nhwc.
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

// ------------------------------------------------------------------------------------------------------------
// training stem: conv1 raw + per-tile BatchNorm statistics, one workgroup per band of k stem rows
// ------------------------------------------------------------------------------------------------------------
// Batch statistics must be complete before bn1 + ReLU + pool can run, so the raw map z reaches memory once; this launch writes it and
// the (mean, M2) table of cavp_bn_finalize_tiles in the same pass.  A tile of the table is `rows_per_tile` CONSECUTIVE rows of z viewed
// as [N * Hs * Ws][64]: a workgroup owns a band of k consecutive rows of the flattened stem-row index r = n * Hs + sr (rows_per_tile =
// k * Ws, only the last band partial).  k <= Hs, so a band lies in one image or straddles one image border: its input patch has two
// segments, (2 ka + 5) rows of image n and (2 kb + 5) rows of image n + 1, ka + kb = k.
// Work item = the eval kernel's: 8 output channels x AS_R stem columns of one stem row (48 f32 accumulators); a band has k * strips * 8
// <= 256 of them, ONE per thread, so the values stay in registers for the statistics: sum -> mean -> centred squares (two passes over
// registers, as col_tile_stats_kernel; cancellation-free), each reduced over the lanes of a channel group with shuffles, over the four
// waves through LDS, in a fixed order.  The statistics are taken from the values AS STORED (rounded to bf16 where z is bf16): the
// table then is exactly what the two-launch route (cavp_col_tile_stats over z) computes and what the BatchNorm backward centres z
// with.  (The igemm epilogue takes them from the f32 accumulators; in f32 the two are the same numbers.)
constexpr int AST_MAX_POS = 32;     // (stem row, strip) positions of a band: 32 x 8 channel groups = 256 threads

struct AstLayout { int Hs, Ws, strips, k, bands, IC, PR; };
static bool ast_layout(int N, int Cin, int H, int W, AstLayout* L) {
  if (N <= 0 || H <= 0 || W <= 0 || (Cin != 1 && Cin != 2)) return false;
  L->Hs = (H - 1) / 2 + 1;
  L->Ws = (W - 1) / 2 + 1;
  L->strips = (L->Ws + AS_R - 1) / AS_R;
  if (L->strips > AST_MAX_POS) return false;
  if ((long long)N * L->Hs * L->Ws > 0x7fffffffll) return false;
  int k = AST_MAX_POS / L->strips;
  L->k = k < L->Hs ? k : L->Hs;
  L->bands = (int)(((long long)N * L->Hs + L->k - 1) / L->k);
  L->IC = 2 * (L->strips * AS_R - 1) + 7;     // input columns -3 .. : what the strips read
  L->PR = 2 * L->k + 10;                      // patch rows of both segments
  return true;
}
static size_t ast_lds_bytes(int Cin, const AstLayout& L) {
  return ((size_t)Cin * 49 * AS_CO + 4 * AS_CO + AS_CO + (size_t)Cin * L.PR * L.IC) * sizeof(float);
}

template <typename T> __device__ __forceinline__ float as_stored(float v) {
  if constexpr (std::is_same<T, float>::value) return v;
  else return bf2f(f2bf(v));
}

// sum over the 8 lanes of a wave that share lane & 7 (the work items of one channel group)
__device__ __forceinline__ float ast_group_sum(float v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

template <typename T, int CIN>
__global__ __launch_bounds__(256) void audio_stem_train_kernel(const float* __restrict__ x, const float* __restrict__ w, T* __restrict__ z,
                                                               float* __restrict__ ts, int N, int H, int W, int Hs, int Ws, int k,
                                                               int strips, int bands, int IC, int PR) {
  extern __shared__ __attribute__((aligned(16))) unsigned char as_smem[];
  float* wl = (float*)as_smem;                       // [CIN][7][7][64]
  float* red = wl + CIN * 49 * AS_CO;                // [4 waves][64]
  float* mean_s = red + 4 * AS_CO;                   // [64]
  float* patch = mean_s + AS_CO;                     // [CIN][PR][IC]
  constexpr int VE = VecT<T>::VE;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cg = tid & 7, pos = tid >> 3;
  const int j = pos / strips, c0 = (pos - j * strips) * AS_R;   // stem row of the band, first stem column
  const int R = N * Hs;

  for (int i = tid; i < CIN * 49 * AS_CO; i += 256) {
    const int o = i & (AS_CO - 1), t = i >> 6;
    wl[i] = w[o * (CIN * 49) + t];
  }

  for (int band = blockIdx.x; band < bands; band += gridDim.x) {
    const int r0 = band * k;
    const int na = r0 / Hs, sra0 = r0 - na * Hs;
    const int ka = k < Hs - sra0 ? k : Hs - sra0;     // rows of the band in image na; the rest start image na + 1 at stem row 0
    const int pa = 2 * ka + 5;
    const int prows = ka < k ? PR : pa;
    __syncthreads();                                  // the previous band's reads of patch / red (and, first, the weight writes) are done
    for (int i = tid; i < CIN * prows * IC; i += 256) {
      const int c = i % IC, q = i / IC, p = q % prows, ci = q / prows;
      const int n = p < pa ? na : na + 1;
      const int hi = p < pa ? 2 * sra0 - 3 + p : p - pa - 3, wi = c - 3;
      const bool ok = n < N && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
      patch[(ci * PR + p) * IC + c] = ok ? x[(((size_t)n * CIN + ci) * H + hi) * W + wi] : 0.f;
    }
    __syncthreads();

    int nv = 0;                                       // valid stem columns of this work item
    if (j < k && r0 + j < R) nv = Ws - c0 < AS_R ? Ws - c0 : AS_R;
    float v[AS_R][8];
#pragma unroll
    for (int r = 0; r < AS_R; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[r][e] = 0.f;
    if (nv > 0) {
      const int prow0 = j < ka ? 2 * j : pa + 2 * (j - ka);
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) {
#pragma unroll 1
        for (int kh = 0; kh < 7; ++kh) {
          const float* prow = patch + (ci * PR + prow0 + kh) * IC + 2 * c0;
          float in[2 * (AS_R - 1) + 7];
#pragma unroll
          for (int u = 0; u < 2 * (AS_R - 1) + 7; ++u) in[u] = prow[u];
          const float* wrow = wl + ((ci * 7 + kh) * 7) * AS_CO + cg * 8;
#pragma unroll
          for (int kw = 0; kw < 7; ++kw) {
            const float4 wa = *(const float4*)(wrow + kw * AS_CO), wb = *(const float4*)(wrow + kw * AS_CO + 4);
            const float wv8[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int r = 0; r < AS_R; ++r)
#pragma unroll
              for (int e = 0; e < 8; ++e) v[r][e] = fmaf(in[2 * r + kw], wv8[e], v[r][e]);
          }
        }
      }
      T* zp = z + ((size_t)(r0 + j) * Ws + c0) * AS_CO + cg * 8;
#pragma unroll
      for (int r = 0; r < AS_R; ++r) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[r][e] = as_stored<T>(v[r][e]);
        if (r < nv) {
#pragma unroll
          for (int e = 0; e < 8; e += VE) VecT<T>::store(zp + (size_t)r * AS_CO + e, v[r] + e);
        }
      }
    }

    // tile statistics of the stored values: sum -> mean -> centred squares
    const int rows_b = R - r0 < k ? R - r0 : k;
    const float cnt = (float)(rows_b * Ws);
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] = 0.f;
#pragma unroll
      for (int r = 0; r < AS_R; ++r) s[e] += r < nv ? v[r][e] : 0.f;
      s[e] = ast_group_sum(s[e]);
    }
    if (lane < 8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wv * AS_CO + cg * 8 + e] = s[e];
    }
    __syncthreads();
    if (tid < AS_CO) mean_s[tid] = (red[tid] + red[AS_CO + tid] + red[2 * AS_CO + tid] + red[3 * AS_CO + tid]) / cnt;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float m = mean_s[cg * 8 + e];
      float q = 0.f;
#pragma unroll
      for (int r = 0; r < AS_R; ++r) {
        const float d = r < nv ? v[r][e] - m : 0.f;
        q = fmaf(d, d, q);
      }
      s[e] = ast_group_sum(q);
    }
    if (lane < 8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wv * AS_CO + cg * 8 + e] = s[e];
    }
    __syncthreads();
    if (tid < AS_CO)
      *(float2*)(ts + ((size_t)band * AS_CO + tid) * 2) =
          make_float2(mean_s[tid], red[tid] + red[AS_CO + tid] + red[2 * AS_CO + tid] + red[3 * AS_CO + tid]);
  }
}

extern "C" int cavp_audio_stem_train_layout(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t* tiles, int32_t* rows_per_tile) {
  AstLayout L;
  if (!tiles || !rows_per_tile || !ast_layout(N, Cin, H, W, &L) || ast_lds_bytes(Cin, L) > 64 * 1024) return 0;
  *tiles = L.bands;
  *rows_per_tile = L.k * L.Ws;
  return 1;
}

template <typename T, int CIN>
static bool audio_stem_train_launch(const float* x, const float* w, void* z, float* ts, int N, int H, int W, const AstLayout& L, hipStream_t s) {
  // (up to 64 KiB of dynamic LDS: 38 KiB for stereo 300 x 64 clips, four workgroups per CU; asked for once per instantiation - if the
  // runtime refuses, nothing is launched: a launch above the default limit would only fail later, with a less telling error)
  static const hipError_t once = hipFuncSetAttribute((const void*)audio_stem_train_kernel<T, CIN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     64 * 1024);
  if (once != hipSuccess) return false;
  const int nb = L.bands < 1024 ? L.bands : 1024;     // the weights are staged once per workgroup, which then walks the bands
  audio_stem_train_kernel<T, CIN><<<nb, 256, ast_lds_bytes(CIN, L), s>>>(x, w, (T*)z, ts, N, H, W, L.Hs, L.Ws, L.k, L.strips, L.bands, L.IC, L.PR);
  return true;
}

extern "C" int cavp_audio_stem_train(int32_t dtype, const float* x_nchw, const float* w_oihw, void* z_nhwc, float* tile_stats, int32_t N,
                                     int32_t Cin, int32_t H, int32_t W, void* stream) {
  if (!x_nchw || !w_oihw || !z_nhwc || !tile_stats || N <= 0 || H <= 0 || W <= 0) return CAVP_ERR_BAD_ARG;
  if (!dt_ok(dtype)) return CAVP_ERR_UNSUPPORTED;
  AstLayout L;
  if (!ast_layout(N, Cin, H, W, &L) || ast_lds_bytes(Cin, L) > 64 * 1024) return CAVP_ERR_UNSUPPORTED;
  if (!al16(z_nhwc) || ((uintptr_t)tile_stats & 7)) return CAVP_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  bool launched = false;
  cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
    launched = Cin == 1 ? audio_stem_train_launch<T, 1>(x_nchw, w_oihw, z_nhwc, tile_stats, N, H, W, L, s)
                        : audio_stem_train_launch<T, 2>(x_nchw, w_oihw, z_nhwc, tile_stats, N, H, W, L, s); });
  if (!launched) return CAVP_ERR_LAUNCH;
  CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// global max with its winner, and the backward through it
// ------------------------------------------------------------------------------------------------------------
// gmp_kernel's walk (grid (channel block, n), four waves stride over the rows) carrying the position: a wave keeps the FIRST maximum of
// the rows it visits (strict >, ascending i), the four are merged by (larger value, then smaller position) = nn.AdaptiveMaxPool2d's
// winner, the first maximum in (h, w) scan order.  A NaN wins as in torch (`val > max || isnan(val)`): the result is NaN and the
// winner the LAST NaN in scan order.  (The eval launch gmp_kernel above keeps fmaxf, which drops a NaN.)
__device__ __forceinline__ bool gmp_takes(float pv, int pi, float m, int a) {
  if (pv != pv) return m == m || pi > a;
  if (m != m) return false;
  return pv > m || (pv == m && pi < a);
}
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gmp_arg_kernel(const T* __restrict__ x, T* __restrict__ y, int* __restrict__ arg, int HW, int C,
                                                      int ldx) {
  constexpr int VE = VEC ? VecT<T>::VE : 1;
  __shared__ float part[4][64 * VE];
  __shared__ int parti[4][64 * VE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.y, c = (blockIdx.x * 64 + lane) * VE;
  float m[VE];
  int a[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) { m[j] = -INFINITY; a[j] = 0; }
  if (c < C) {
    const T* xp = x + (size_t)n * HW * ldx + c;
    for (int i = wv; i < HW; i += 4) {
      float v[VE];
      if constexpr (VEC) VecT<T>::load(xp + (size_t)i * ldx, v);
      else v[0] = Elem<T>::ld(xp + (size_t)i * ldx);
#pragma unroll
      for (int j = 0; j < VE; ++j)
        if (v[j] > m[j] || v[j] != v[j]) { m[j] = v[j]; a[j] = i; }
    }
  }
#pragma unroll
  for (int j = 0; j < VE; ++j) { part[wv][j * 64 + lane] = m[j]; parti[wv][j * 64 + lane] = a[j]; }
  __syncthreads();
  if (wv == 0 && c < C) {
#pragma unroll
    for (int j = 0; j < VE; ++j) {
#pragma unroll
      for (int q = 1; q < 4; ++q) {
        const float pv = part[q][j * 64 + lane];
        const int pi = parti[q][j * 64 + lane];
        if (gmp_takes(pv, pi, m[j], a[j])) { m[j] = pv; a[j] = pi; }
      }
    }
    T* yp = y + (size_t)n * C + c;
    int* ap = arg + (size_t)n * C + c;
    if constexpr (VEC) VecT<T>::store(yp, m);
    else Elem<T>::st(yp, m[0]);
#pragma unroll
    for (int j = 0; j < VE; ++j) ap[j] = a[j];
  }
}

extern "C" int cavp_global_maxpool_arg_nhwc(int32_t dtype, const void* x, void* y, int32_t* arg, int32_t N, int32_t HW, int32_t C,
                                            int32_t ldx, void* stream) {
  if (!x || !y || !arg || N <= 0 || HW <= 0 || C <= 0 || ldx < C) return CAVP_ERR_BAD_ARG;
  if (!dt_ok(dtype)) return CAVP_ERR_UNSUPPORTED;
  if (N > 65535) return CAVP_ERR_UNSUPPORTED;
  const int VE = dt_ve(dtype);
  const bool vec = C % VE == 0 && ldx % VE == 0 && al16(x) && al16(y);
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
    cavp_dispatch_bool(vec, [&](auto v) {
      constexpr bool V = decltype(v)::value;
      const int per = 64 * (V ? (int)VecT<T>::VE : 1);
      gmp_arg_kernel<T, V><<<dim3((C + per - 1) / per, N), 256, 0, s>>>((const T*)x, (T*)y, arg, HW, C, ldx); }); });
  CHECK_LAUNCH();
}

// dx[n][i][c] = arg[n][c] == i ? dy[n][c] : 0 for EVERY (i, c): one pass, no zero fill in front of it.  grid (blocks over HW x channel
// vectors, n); a thread owns one channel vector (VEC) or one channel of one position.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gmp_bwd_kernel(const int* __restrict__ arg, const T* __restrict__ dy, T* __restrict__ dx, int HW,
                                                      int C) {
  constexpr int VE = VEC ? VecT<T>::VE : 1;
  const int CV = C / VE, n = blockIdx.y;
  const long long total = (long long)HW * CV;   // (64-bit walk: HW * C may be within one grid stride of 2^31)
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int i = (int)(idx / CV), c = (int)(idx - (long long)i * CV) * VE;
    const int* ap = arg + (size_t)n * C + c;
    float g[VE], o[VE];
    if constexpr (VEC) VecT<T>::load(dy + (size_t)n * C + c, g);
    else g[0] = Elem<T>::ld(dy + (size_t)n * C + c);
#pragma unroll
    for (int j = 0; j < VE; ++j) o[j] = ap[j] == i ? g[j] : 0.f;
    T* op = dx + ((size_t)n * HW + i) * C + c;
    if constexpr (VEC) VecT<T>::store(op, o);
    else Elem<T>::st(op, o[0]);
  }
}

extern "C" int cavp_global_maxpool_bwd_nhwc(int32_t dtype, const int32_t* arg, const void* dy, void* dx, int32_t N, int32_t HW, int32_t C,
                                            void* stream) {
  if (!arg || !dy || !dx || N <= 0 || HW <= 0 || C <= 0) return CAVP_ERR_BAD_ARG;
  if (!dt_ok(dtype)) return CAVP_ERR_UNSUPPORTED;
  if (N > 65535 || (long long)HW * C > 0x7fffffffll) return CAVP_ERR_UNSUPPORTED;
  const int VE = dt_ve(dtype);
  const bool vec = C % VE == 0 && al16(dy) && al16(dx);
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
    cavp_dispatch_bool(vec, [&](auto v) {
      constexpr bool V = decltype(v)::value;
      const long long total = (long long)HW * (C / (V ? (int)VecT<T>::VE : 1));
      long long nb = (total + 255) / 256;
      if (nb > 4096) nb = 4096;
      gmp_bwd_kernel<T, V><<<dim3((unsigned)nb, N), 256, 0, s>>>(arg, (const T*)dy, (T*)dx, HW, C); }); });
  CHECK_LAUNCH();
}
