// Image labels from the pixel labels on the device (include/cavp_hip.h, "label stage"): what the reference's data sets compute
// after the transform - the VPO class-index remap of the mask (vpo_mono/multi_source/visual/visual_dataset.py:127-145), the class
// vector one_hot(unique(label[label != 255])).sum(0), the AVSS binary collapse (avss/visual/visual_dataset.py:157-165) and
// AVSBench's one_hot(mask.sum() != 0, 2) (avsbench_ms.py:135-136) - as two or three launches with no host value that depends on
// a device value.  presence (only with a remap) -> scan -> expand.  Which values an image holds is a 256-bit mask per image, ORed
// together in LDS per workgroup and with at most eight 32-bit global atomicOr per workgroup: order-independent, bit-reproducible.
#include "host_util.h"

constexpr int kLabMaxB = 1024;
constexpr int kLabMaxK = 256;
constexpr int kLabWords = 8;                 // 256 bits per image
// an entry of the per-image rule table: bits 0..7 the value written, bits 8..16 the class bit to set (256 = none), bit 17 bad
constexpr unsigned kLutBad = 1u << 17;

// ---- presence: one bit per value a workgroup has seen, a read before the atomic (labels are patches of one value: the read is a
// broadcast and the atomic is rare); `last` spares even the read while the thread stays inside a patch
__device__ __forceinline__ void lab_mark(unsigned* smask, unsigned bit, unsigned& last) {
  if (bit == last) return;
  last = bit;
  const unsigned w = bit >> 5, m = 1u << (bit & 31);
  if (!(smask[w] & m)) atomicOr(&smask[w], m);
}

// the workgroup's mask into the image's (zero at rest: the expand kernel clears it after reading)
__device__ __forceinline__ void lab_flush(const unsigned* smask, unsigned* __restrict__ gmask) {
  __syncthreads();
  if (threadIdx.x < kLabWords) {
    const unsigned m = smask[threadIdx.x];
    if (m) atomicOr(&gmask[threadIdx.x], m);
  }
}

// i-th 16-byte group of a row as pixel values: 2 of int64, 16 of uint8
__device__ __forceinline__ void lab_load16(const long long* row, long long i, long long (&v)[2]) {
  const uint4 q = ((const uint4*)row)[i];
  v[0] = (long long)(((unsigned long long)q.y << 32) | q.x);
  v[1] = (long long)(((unsigned long long)q.w << 32) | q.z);
}
__device__ __forceinline__ void lab_load16(const unsigned char* row, long long i, long long (&v)[16]) {
  const uint4 q = ((const uint4*)row)[i];
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = (long long)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
}

template <typename T> struct LabVec;
template <> struct LabVec<long long> { static constexpr int N = 2; };
template <> struct LabVec<unsigned char> { static constexpr int N = 16; };

// raw_mask[b] |= the values in [0, 256) of image b (a value outside is no key of the remap table: the scan counts it)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void labels_presence_kernel(const T* __restrict__ label, long long HW, unsigned* __restrict__ raw_mask) {
  __shared__ unsigned smask[kLabWords];
  const int b = blockIdx.y;
  if (threadIdx.x < kLabWords) smask[threadIdx.x] = 0u;
  __syncthreads();
  const T* row = label + (size_t)b * HW;
  unsigned last = ~0u;
  const long long step = (long long)gridDim.x * 256;
  if (VEC) {
    constexpr int N = LabVec<T>::N;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW / N; i += step) {
      long long v[N];
      lab_load16(row, i, v);
#pragma unroll
      for (int j = 0; j < N; ++j)
        if ((unsigned long long)v[j] < 256ull) lab_mark(smask, (unsigned)v[j], last);
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += step) {
      const long long v = (long long)row[i];
      if ((unsigned long long)v < 256ull) lab_mark(smask, (unsigned)v, last);
    }
  }
  lab_flush(smask, raw_mask + (size_t)b * kLabWords);
}

// What the rules make of raw value v of this image: the value written, the class bit, the bad flag.
//   remap: the reference's loop `for i in unique(label) \ {0, ignore}, ascending: label[label == i] = remap[i]` runs in place over
//   a value list taken before it, so a pixel moved to t > i is moved again at step t when t was in the raw image.  Per value:
//   x = v; t = remap[x]; while t > x and t was present and is neither 0 nor ignore: x = t, t = remap[x]; the result is t.  x rises
//   strictly: at most 255 rounds.  remap[x] outside [0, 255] (-1: the reference raises): bad, the pixel keeps x.
__device__ __forceinline__ unsigned lab_rule(int v, const int* __restrict__ remap, const unsigned* present, int K, int any_fg,
                                             int binary, long long ignore) {
  int f = v;
  bool bad = false;
  if (remap && v != 0 && (long long)v != ignore) {
    int x = v;
    for (int round = 0; round < 256; ++round) {
      const int t = remap[x];
      if (t < 0 || t > 255) { bad = true; f = x; break; }
      f = t;
      if (t > x && t != 0 && (long long)t != ignore && ((present[t >> 5] >> (t & 31)) & 1u)) x = t; else break;
    }
  }
  unsigned bit = 256u;
  if (any_fg) {
    bit = f != 0 ? 1u : 0u;
  } else if ((long long)f != ignore) {
    if (f < K) bit = (unsigned)f; else bad = true;
  }
  const int out = (binary && f != 0 && (long long)f != ignore) ? 1 : f;
  return (unsigned)out | (bit << 8) | (bad ? kLutBad : 0u);
}

// a pixel value outside [0, 256) (int64 input only): no key of the remap table and no class (K <= 256), so it is bad unless it is
// the ignore value; it keeps its value, collapses to 1 like any other non-zero, and is "non-zero" for any_foreground
__device__ __forceinline__ long long lab_outside(long long v, int any_fg, int has_remap, int binary, long long ignore, unsigned& bit,
                                                 unsigned& bad) {
  const bool ign = v == ignore;
  bit = any_fg ? 1u : 256u;
  bad += (any_fg ? (has_remap && !ign) : !ign) ? 1u : 0u;
  return (binary && !ign) ? 1ll : v;
}

// mask[b] |= the class bits of image b after remap, bad pixels counted into state[0], out (optional) = the remapped / collapsed
// int64 copy.  The 256-entry rule table is built once per workgroup from the raw presence mask; a pixel is one LDS lookup.
template <typename T, bool VEC, bool WRITE>
__global__ __launch_bounds__(256) void labels_scan_kernel(const T* __restrict__ label, long long HW, int K, int any_fg,
                                                          const int* __restrict__ remap, int binary, long long ignore,
                                                          const unsigned* __restrict__ raw_mask, unsigned* __restrict__ mask,
                                                          long long* __restrict__ state, long long* __restrict__ out) {
  __shared__ unsigned smask[kLabWords];
  __shared__ unsigned spresent[kLabWords];
  __shared__ unsigned lut[256];
  __shared__ unsigned s_bad;
  const int b = blockIdx.y, t = threadIdx.x;
  if (t < kLabWords) {
    smask[t] = 0u;
    spresent[t] = remap ? raw_mask[(size_t)b * kLabWords + t] : 0u;
  }
  if (t == 0) s_bad = 0u;
  __syncthreads();
  lut[t] = lab_rule(t, remap, spresent, K, any_fg, binary, ignore);
  __syncthreads();
  const T* row = label + (size_t)b * HW;
  long long* orow = WRITE ? out + (size_t)b * HW : nullptr;
  unsigned last = ~0u, bad = 0u;
  const int has_remap = remap != nullptr;
  const long long step = (long long)gridDim.x * 256;
  auto pixel = [&](long long v) -> long long {
    unsigned bit;
    long long o;
    if ((unsigned long long)v < 256ull) {
      const unsigned e = lut[(unsigned)v];
      o = (long long)(e & 0xffu);
      bit = (e >> 8) & 0x1ffu;
      bad += (e >> 17) & 1u;
    } else {
      o = lab_outside(v, any_fg, has_remap, binary, ignore, bit, bad);
    }
    if (bit < 256u) lab_mark(smask, bit, last);
    return o;
  };
  if (VEC) {
    constexpr int N = LabVec<T>::N;
    for (long long i = (long long)blockIdx.x * 256 + t; i < HW / N; i += step) {
      long long v[N];
      lab_load16(row, i, v);
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] = pixel(v[j]);
      if (WRITE) {
#pragma unroll
        for (int j = 0; j < N; j += 2) {
          const unsigned long long a = (unsigned long long)v[j], c = (unsigned long long)v[j + 1];
          ((uint4*)orow)[i * (N / 2) + j / 2] = make_uint4((unsigned)a, (unsigned)(a >> 32), (unsigned)c, (unsigned)(c >> 32));
        }
      }
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + t; i < HW; i += step) {
      const long long o = pixel((long long)row[i]);
      if (WRITE) orow[i] = o;
    }
  }
  if (bad) atomicAdd(&s_bad, bad);
  lab_flush(smask, mask + (size_t)b * kLabWords);   // (its barrier also orders s_bad)
  if (t == 0 && s_bad) atomicAdd((unsigned long long*)state, (unsigned long long)s_bad);
}

// img_label[b][c] = bit c of mask[b] (any_foreground: [no bit 1, bit 1]); then both masks of the image are cleared for the next call
__global__ __launch_bounds__(kLabMaxK) void labels_expand_kernel(unsigned* __restrict__ mask, unsigned* __restrict__ raw_mask, int K,
                                                                 int any_fg, long long* __restrict__ img_label) {
  __shared__ unsigned sm[kLabWords];
  const int b = blockIdx.x, c = threadIdx.x;
  if (c < kLabWords) sm[c] = mask[(size_t)b * kLabWords + c];
  __syncthreads();
  if (c < K) {
    long long v;
    if (any_fg)
      v = (long long)(((sm[0] >> 1) & 1u) == (unsigned)(c == 1)) * (c < 2);
    else
      v = (long long)((sm[c >> 5] >> (c & 31)) & 1u);
    img_label[(size_t)b * K + c] = v;
  }
  if (c < kLabWords) {
    mask[(size_t)b * kLabWords + c] = 0u;
    if (raw_mask) raw_mask[(size_t)b * kLabWords + c] = 0u;
  }
}

// workgroups per image: 256 threads x 4 accesses each, at most 64 per image
static inline unsigned labels_row_blocks(long long accesses) {
  long long nb = (accesses + 1023) / 1024;
  return (unsigned)(nb < 1 ? 1 : nb > 64 ? 64 : nb);
}

static inline bool labels_vec_ok(const void* label, int is_u8, long long HW) {
  return al16(label) && HW % (is_u8 ? 16 : 2) == 0;
}

extern "C" int cavp_labels_presence(const void* label, int32_t label_u8, int32_t B, int64_t HW, uint32_t* raw_mask, void* stream) {
  if (!label || !raw_mask || B < 1 || HW < 1) return CAVP_ERR_BAD_ARG;
  if (B > kLabMaxB) return CAVP_ERR_UNSUPPORTED;
  const bool vec = labels_vec_ok(label, label_u8, HW);
  const dim3 grid(labels_row_blocks(vec ? HW / (label_u8 ? 16 : 2) : HW), B);
  hipStream_t s = (hipStream_t)stream;
  if (label_u8) {
    if (vec) labels_presence_kernel<unsigned char, true><<<grid, 256, 0, s>>>((const unsigned char*)label, HW, raw_mask);
    else labels_presence_kernel<unsigned char, false><<<grid, 256, 0, s>>>((const unsigned char*)label, HW, raw_mask);
  } else {
    if (vec) labels_presence_kernel<long long, true><<<grid, 256, 0, s>>>((const long long*)label, HW, raw_mask);
    else labels_presence_kernel<long long, false><<<grid, 256, 0, s>>>((const long long*)label, HW, raw_mask);
  }
  CHECK_LAUNCH();
}

template <typename T>
static void labels_scan_launch(const T* label, long long HW, int B, int K, int any_fg, const int* remap, int binary, long long ignore,
                               const unsigned* raw_mask, unsigned* mask, long long* state, long long* out, bool vec, hipStream_t s) {
  const dim3 grid(labels_row_blocks(vec ? HW / LabVec<T>::N : HW), B);
  if (vec && out) labels_scan_kernel<T, true, true><<<grid, 256, 0, s>>>(label, HW, K, any_fg, remap, binary, ignore, raw_mask, mask, state, out);
  else if (vec) labels_scan_kernel<T, true, false><<<grid, 256, 0, s>>>(label, HW, K, any_fg, remap, binary, ignore, raw_mask, mask, state, out);
  else if (out) labels_scan_kernel<T, false, true><<<grid, 256, 0, s>>>(label, HW, K, any_fg, remap, binary, ignore, raw_mask, mask, state, out);
  else labels_scan_kernel<T, false, false><<<grid, 256, 0, s>>>(label, HW, K, any_fg, remap, binary, ignore, raw_mask, mask, state, out);
}

extern "C" int cavp_labels_scan(const void* label, int32_t label_u8, int32_t B, int64_t HW, int32_t K, int32_t any_foreground,
                                const int32_t* remap, int32_t binary, int64_t ignore, const uint32_t* raw_mask, uint32_t* mask,
                                int64_t* state, int64_t* out_label, void* stream) {
  if (!label || !mask || !state || B < 1 || HW < 1 || K < 1 || (remap && !raw_mask)) return CAVP_ERR_BAD_ARG;
  if (B > kLabMaxB || K > kLabMaxK || (any_foreground && K != 2)) return CAVP_ERR_UNSUPPORTED;
  const bool vec = labels_vec_ok(label, label_u8, HW) && (!out_label || al16(out_label));
  hipStream_t s = (hipStream_t)stream;
  if (label_u8)
    labels_scan_launch((const unsigned char*)label, HW, B, K, any_foreground ? 1 : 0, remap, binary ? 1 : 0, ignore, raw_mask, mask,
                       (long long*)state, (long long*)out_label, vec, s);
  else
    labels_scan_launch((const long long*)label, HW, B, K, any_foreground ? 1 : 0, remap, binary ? 1 : 0, ignore, raw_mask, mask,
                       (long long*)state, (long long*)out_label, vec, s);
  CHECK_LAUNCH();
}

extern "C" int cavp_labels_expand(uint32_t* mask, uint32_t* raw_mask, int32_t B, int32_t K, int32_t any_foreground, int64_t* img_label,
                                  void* stream) {
  if (!mask || !img_label || B < 1 || K < 1) return CAVP_ERR_BAD_ARG;
  if (B > kLabMaxB || K > kLabMaxK || (any_foreground && K != 2)) return CAVP_ERR_UNSUPPORTED;
  labels_expand_kernel<<<B, kLabMaxK, 0, (hipStream_t)stream>>>(mask, raw_mask, K, any_foreground ? 1 : 0, (long long*)img_label);
  CHECK_LAUNCH();
}
