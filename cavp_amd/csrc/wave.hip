// Wave stage on the device (include/cavp_hip.h, "wave stage"): the mono 16 kHz window the reference's data sets cut on the host
// (Resample -> crop_audio -> sum over sources / mean over channels -> one second of a clip; vpo_mono/multi_source/audio/
// audio_dataset.py:48-70, avss/audio/audio_dataset.py:42-62, avsbench_ms.py:129-134,156-159,169-180) as one launch.  Only the
// cropped window of the resampled signal is ever computed: a gather-FIR of `span` taps per output.
#include "host_util.h"

constexpr int kWaveTile = 1024;                           // consecutive outputs of one row per workgroup
constexpr int kWaveThreads = 256;
constexpr int kWavePer = kWaveTile / kWaveThreads;        // outputs per thread: a, a + 256, ... (adjacent lanes, adjacent phases)
constexpr int kWaveMaxLds = 160 * 1024;
constexpr long long kWaveMaxLen = 1ll << 28;              // L16 <= 4 L < 2^31: the positions in y are 32-bit, the products are not

struct WaveRate {   // one row of rate_desc
  int o, n, span, stride, tap_off, first_off, shift, fspread;
};

__device__ __forceinline__ float wave_sample(const float* p) { return *p; }
__device__ __forceinline__ float wave_sample(const short* p) { return (float)*p * (1.0f / 32768.0f); }

// the three LDS capacities hold this rate for any tile (the x span of at most kWaveTile consecutive positions of y)
__device__ __forceinline__ bool wave_rate_fits(const WaveRate& d, int tab_cap, int first_cap, int x_cap) {
  if (d.o < 1 || d.n < 1 || d.span < 1 || d.stride < d.span || d.fspread < 0 || d.tap_off < 0 || d.first_off < 0) return false;
  const long long x = ((long long)(kWaveTile - 1) / d.n + 1) * d.o + d.fspread + d.span;
  return (long long)d.n * d.stride <= tab_cap && d.n <= first_cap && x <= x_cap;
}

// grid (tiles, B).  The workgroup loops over the sources and channels of its row; per source it stages the rate's compact filter
// (only when the rate changes) and per channel the input span of its tile, zero outside [0, L), in LDS.  A short clip repeats
// (i % ln): a tile then covers one or two contiguous ranges of y, each staged and computed in a pass of its own.
template <typename T>
__global__ __launch_bounds__(kWaveThreads) void wave_stage_kernel(const T* __restrict__ raw, const int* __restrict__ length,
                                                                  const int* __restrict__ rate_idx, const int* __restrict__ n_ch,
                                                                  const int* __restrict__ select, int S, int C, long long Lmax,
                                                                  int sample_len, int segments, const WaveRate* __restrict__ rates,
                                                                  int n_rates, const float* __restrict__ taps,
                                                                  const int* __restrict__ first, int tab_cap, int first_cap, int x_cap,
                                                                  unsigned long long* __restrict__ state, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_tab = (float*)smem;
  int* s_first = (int*)(s_tab + tab_cap);
  float* s_x = (float*)(s_first + first_cap);
  const int b = blockIdx.y, t = threadIdx.x;
  const int A_out = select ? sample_len / segments : sample_len;
  const int tile0 = blockIdx.x * kWaveTile;
  const int nt = min(kWaveTile, A_out - tile0);
  float* orow = out + (size_t)b * A_out + tile0;

  // ---- the row's inputs, checked by every workgroup of the row (uniform), counted by the first
  int bad = 0, woff = 0;
  if (select) {
    const int sel = select[b];
    if (sel < 0 || sel >= segments)
      ++bad;
    else
      woff = sel * A_out;
  }
  for (int s = 0; s < S; ++s) {
    const int L = length[b * S + s];
    if (L < 0 || L > Lmax) {
      ++bad;
    } else if (L > 0) {
      const int r = rate_idx[b * S + s], nc = n_ch[b * S + s];
      if (r < 0 || r >= n_rates || !wave_rate_fits(rates[r], tab_cap, first_cap, x_cap)) ++bad;
      if (nc < 1 || nc > C) ++bad;
    }
  }
  if (bad) {
    if (blockIdx.x == 0 && t == 0) atomicAdd(state, (unsigned long long)bad);
#pragma unroll
    for (int q = 0; q < kWavePer; ++q) {
      const int a = t + q * kWaveThreads;
      if (a < nt) orow[a] = 0.0f;
    }
    return;
  }

  const int i0 = woff + tile0;   // first position of the tile in the row's window of sample_len values
  float acc[kWavePer];
#pragma unroll
  for (int q = 0; q < kWavePer; ++q) acc[q] = 0.0f;
  int cur_rate = -1;
  for (int s = 0; s < S; ++s) {
    const int L = length[b * S + s];
    if (L == 0) continue;
    const int r = rate_idx[b * S + s], nc = n_ch[b * S + s];
    const WaveRate d = rates[r];
    if (r != cur_rate) {   // (every pass below ends with a barrier: nobody still reads the old filter)
      const int words = d.n * d.stride;
      for (int i = t; i < words; i += kWaveThreads) s_tab[i] = taps[d.tap_off + i];
      for (int i = t; i < d.n; i += kWaveThreads) s_first[i] = first[d.first_off + i];
      cur_rate = r;
    }
    // ---- crop_audio's slice of the resampled signal
    const long long L16 = ((long long)d.n * L + d.o - 1) / d.o;
    const long long st = L16 / 2 - sample_len / 2;
    const long long s0 = st >= 0 ? st : (L16 + st > 0 ? L16 + st : 0);
    const long long s1 = st + sample_len < L16 ? st + sample_len : L16;
    const int ln = s1 - s0 >= 1 ? (int)(s1 - s0) : 1;
    const bool whole = ln == sample_len;
    // ---- the tile's ranges [ra, rb) of offsets into the slice
    int ra[2], rb[2];
    ra[1] = rb[1] = 0;
    if (ln <= kWaveTile) {
      ra[0] = 0;
      rb[0] = ln;
    } else {
      const int r0 = whole ? i0 : i0 % ln;
      ra[0] = r0;
      rb[0] = min(ln, r0 + nt);
      rb[1] = r0 + nt - rb[0];
    }
    const int npass = rb[1] > 0 ? 2 : 1;
    float wsum[kWavePer];
#pragma unroll
    for (int q = 0; q < kWavePer; ++q) wsum[q] = 0.0f;
    for (int c = 0; c < nc; ++c) {
      const T* src = raw + ((size_t)(b * S + s) * C + c) * (size_t)Lmax;
      for (int ps = 0; ps < npass; ++ps) {
        const unsigned ja = (unsigned)(s0 + ra[ps]), jl = (unsigned)(s0 + rb[ps] - 1);
        const unsigned qa = ja / (unsigned)d.n, qb = jl / (unsigned)d.n;
        const long long xlo = (long long)qa * d.o + d.shift;
        const int xcount = (int)(qb - qa) * d.o + d.fspread + d.span;   // <= x_cap (wave_rate_fits)
        for (int i = t; i < xcount; i += kWaveThreads) {
          const long long g = xlo + i;
          s_x[i] = (g >= 0 && g < L) ? wave_sample(src + g) : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kWavePer; ++q) {
          const int a = t + q * kWaveThreads;
          if (a < nt) {
            const int i = i0 + a;
            const int rr = whole ? i : i % ln;
            if (rr >= ra[ps] && rr < rb[ps]) {
              const unsigned j = (unsigned)(s0 + rr);
              const unsigned qq = j / (unsigned)d.n;
              const int p = (int)(j - qq * (unsigned)d.n);
              const float* h = s_tab + p * d.stride;
              const float* x = s_x + (int)(qq - qa) * d.o + s_first[p];
              float y = h[0] * x[0];
              for (int k = 1; k < d.span; ++k) y = fmaf(h[k], x[k], y);
              wsum[q] += y;
            }
          }
        }
        __syncthreads();
      }
    }
    const float fn = (float)nc;
#pragma unroll
    for (int q = 0; q < kWavePer; ++q) acc[q] += wsum[q] / fn;
  }
#pragma unroll
  for (int q = 0; q < kWavePer; ++q) {
    const int a = t + q * kWaveThreads;
    if (a < nt) orow[a] = acc[q];
  }
}

// past the 64 KiB default; once per instantiation
template <typename T>
static void wave_allow_lds() {
  static const hipError_t once =
      hipFuncSetAttribute((const void*)wave_stage_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, kWaveMaxLds);
  (void)once;
}

extern "C" int cavp_wave_tile(void) { return kWaveTile; }

extern "C" int cavp_wave_stage(const void* raw, int32_t raw_i16, const int32_t* length, const int32_t* rate_idx, const int32_t* n_ch,
                               const int32_t* select, int32_t B, int32_t S, int32_t C, int64_t Lmax, int32_t sample_len,
                               int32_t segments, const int32_t* rate_desc, int32_t n_rates, const float* taps, const int32_t* first,
                               int32_t tab_cap, int32_t first_cap, int32_t x_cap, int64_t* state, float* out, void* stream) {
  if (!raw || !length || !rate_idx || !n_ch || !rate_desc || !taps || !first || !state || !out) return CAVP_ERR_BAD_ARG;
  if (B < 1 || S < 1 || C < 1 || Lmax < 1 || sample_len < 1 || segments < 1 || n_rates < 1 || tab_cap < 1 || first_cap < 1 || x_cap < 1)
    return CAVP_ERR_BAD_ARG;
  if (sample_len % segments != 0 || (select && segments < 2)) return CAVP_ERR_BAD_ARG;
  if (B > 65535 || Lmax > kWaveMaxLen || (long long)B * S > 0x7fffffffll) return CAVP_ERR_UNSUPPORTED;
  const size_t lds = ((size_t)tab_cap + (size_t)first_cap + (size_t)x_cap) * 4;
  if (lds > (size_t)kWaveMaxLds) return CAVP_ERR_UNSUPPORTED;
  if (((uintptr_t)state & 7) || ((uintptr_t)out & 3) || ((uintptr_t)raw & (raw_i16 ? 1 : 3))) return CAVP_ERR_ALIGN;
  const int A_out = select ? sample_len / segments : sample_len;
  const dim3 grid((unsigned)((A_out + kWaveTile - 1) / kWaveTile), (unsigned)B);
  if (raw_i16) {
    wave_allow_lds<short>();
    wave_stage_kernel<short><<<grid, kWaveThreads, lds, (hipStream_t)stream>>>(
        (const short*)raw, length, rate_idx, n_ch, select, S, C, (long long)Lmax, sample_len, segments, (const WaveRate*)rate_desc,
        n_rates, taps, first, tab_cap, first_cap, x_cap, (unsigned long long*)state, out);
  } else {
    wave_allow_lds<float>();
    wave_stage_kernel<float><<<grid, kWaveThreads, lds, (hipStream_t)stream>>>(
        (const float*)raw, length, rate_idx, n_ch, select, S, C, (long long)Lmax, sample_len, segments, (const WaveRate*)rate_desc,
        n_rates, taps, first, tab_cap, first_cap, x_cap, (unsigned long long*)state, out);
  }
  CHECK_LAUNCH();
}
