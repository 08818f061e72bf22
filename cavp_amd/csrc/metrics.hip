// Validation metrics for gfx950: the integer counts behind the reference's MIoU / ForegroundDetect (utils/eval_utils.py) and
// mask_iou / Eval_Fmeasure (utils/avsbench_utils.py).  Every kernel streams its input once and accumulates integer counts with
// integer atomics, so a result does not depend on the order in which workgroups arrive: bit-reproducible without
// cavp_set_deterministic.  The float finalisation (IoU, F-beta, precision / recall curves) stays in cavp_amd/metrics.py, in the
// reference's own expressions.
//
//   seg_confusion: argmax over C per pixel (first maximal index, a NaN counts as the maximum: torch.max), then one count in the
//                  (K+1) x K matrix M[row(t)][p] for every pixel whose label t >= 0 and t != ignore; row(t) = t < K ? t : K.
//                  Privatised per workgroup as u32 in LDS when (K+1)*K*4 <= 64 KiB (K <= 127), flushed with one u64 atomic per
//                  non-zero bin; larger K adds straight into M.  The background-correct bin takes most pixels: equal bins are
//                  merged inside a thread's 4 pixels, and the first bin of the wave is summed across the wave (three ballots)
//                  before its one atomic.
//   seg_predict:   the same argmax and counts (and a u8 mask / a softmax-channel probability map) from the model's low-resolution NHWC
//                  logits: the bilinear upsample is evaluated per pixel in registers, the full-resolution tensor is never written.
//   mask_iou_stats: per image  sum p*t, sum max(p, t), sum (1-t)(1-p), sum t  in int64.
//   fmeasure_hist:  per image a (pr_num+1)-bin histogram of bin(p) = #{i : th[i] <= p} over all pixels and over gt != 0;
//                  suffix sums of it are Eval_Fmeasure's y_temp.sum() and tp for every threshold.
//   clipval:       the frames of a batch of clips routed into an ALL and a multi-source confusion matrix: per frame a 256-bin label
//                  histogram and the seg_confusion counts in scratch, then a flag per frame from its histogram and the adds.
//   videoval:      the frames of a batch of videos in one pass: per frame the mask_iou_stats sums and the fmeasure_hist histograms
//                  in scratch, the seg_confusion counts into the global matrix; then one workgroup per video finishes J and F in
//                  float32 (a float tail that runs on the device: per-video scores are stored results).
//   semval:        the per-frame, per-class IoU / F-score of utils/avsbench_metrics.py: per frame the three class-area vectors and the
//                  binary-IoU sums in scratch, then one thread per class adds the frames' float32 scores in ascending order.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBins = 16384;   // 64 KiB of u32 counts

__device__ __forceinline__ void argmax_step(float v, int c, float& best, int& idx) {
  if (v > best || (v != v && best == best)) { best = v; idx = c; }
}

// Add the (bin, count) pairs of one thread's 4 pixels (bin < 0: nothing).  It ballots and shuffles across the wave, so it is called
// by all lanes, once per trip, trip count block-uniform: every kernel below walks its quads as
//   for (base = first quad of the workgroup; base < total; base += quads per grid pass) {
//     q = base + threadIdx.x;  bins = -1;  if (q < total) { bins of quad q }  add_bins(bins);  }
// and never calls it under a per-thread condition (a thread without a quad brings bins of -1).
template <bool kLds, typename G>
__device__ __forceinline__ void add_bins(int b[4], unsigned* lds, G* gM) {
  int cnt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) cnt[i] = b[i] >= 0 ? 1 : 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) {
      if (b[i] >= 0 && b[j] == b[i]) { cnt[j] += cnt[i]; cnt[i] = 0; b[i] = -1; }
    }
  }
  // the wave's first bin (in practice the hot background-correct one): one atomic for the whole wave
  const int first = b[0] >= 0 ? b[0] : (b[1] >= 0 ? b[1] : (b[2] >= 0 ? b[2] : b[3]));
  const unsigned long long any = __ballot(first >= 0);
  if (any) {
    const int lead = __shfl(first, __ffsll((long long)any) - 1, 64);
    int c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (b[i] == lead) { c = cnt[i]; b[i] = -1; }
    }
    const unsigned total = (unsigned)__popcll(__ballot(c & 1)) + 2u * (unsigned)__popcll(__ballot(c & 2)) +
                           4u * (unsigned)__popcll(__ballot(c & 4));
    if ((threadIdx.x & 63) == 0) {
      if (kLds) atomicAdd(lds + lead, total);
      else atomicAdd(gM + lead, (G)total);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (b[i] >= 0) {
      if (kLds) atomicAdd(lds + b[i], (unsigned)cnt[i]);
      else atomicAdd(gM + b[i], (G)cnt[i]);
    }
  }
}

// labels are int64, or float32 holding integers (AVS masks come as float); a non-finite float label is never counted
__device__ __forceinline__ long long label_i64(long long t) { return t; }
__device__ __forceinline__ long long label_i64(float t) { return fabsf(t) <= 9.0e18f ? (long long)t : -1; }

template <typename LT>
__device__ __forceinline__ int conf_bin(LT tv, int p, int K, long long ignore) {
  const long long t = label_i64(tv);
  if (t < 0 || t == ignore) return -1;
  const int row = t < K ? (int)t : K;
  return row * K + p;
}

// ---- one thread's 4 consecutive pixels ("quad") ----------------------------------------------------------------------------------
// kVec: the quad is whole and every array it touches is aligned for one vector access (the host decides); otherwise only its
// first np pixels exist and are accessed one by one.

// pixels of a quad that starts `left` pixels before the end of its image
template <bool kVec>
__device__ __forceinline__ int quad_pixels(long long left) { return kVec ? 4 : (int)(left < 4 ? left : 4); }

// t[j] = p[j] for j < np (0 beyond): two 16-byte loads for int64, one for float32, one 4-byte load for bytes
template <typename LT, bool kVec>
__device__ __forceinline__ void load_quad(const LT* p, int np, LT t[4]) {
  if constexpr (!kVec) {
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = j < np ? p[j] : (LT)0;
  } else if constexpr (sizeof(LT) == 8) {
    const longlong2 t01 = *(const longlong2*)p, t23 = *(const longlong2*)(p + 2);
    t[0] = t01.x; t[1] = t01.y; t[2] = t23.x; t[3] = t23.y;
  } else if constexpr (sizeof(LT) == 4) {
    const float4 t4 = *(const float4*)p;
    t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
  } else {
    const unsigned w = *(const unsigned*)p;
    t[0] = w & 255u; t[1] = (w >> 8) & 255u; t[2] = (w >> 16) & 255u; t[3] = w >> 24;
  }
}

// idx[j] = argmax over the C planes (HW apart) of pixel j of the quad at src: first maximal index, a NaN counts as the maximum
template <bool kVec>
__device__ __forceinline__ void quad_argmax_nchw(const float* src, int C, long long HW, int np, int idx[4]) {
  idx[0] = idx[1] = idx[2] = idx[3] = 0;
  if constexpr (kVec) {
    float4 best = *(const float4*)src;
    for (int c = 1; c < C; ++c) {
      const float4 v = *(const float4*)(src + c * HW);
      argmax_step(v.x, c, best.x, idx[0]);
      argmax_step(v.y, c, best.y, idx[1]);
      argmax_step(v.z, c, best.z, idx[2]);
      argmax_step(v.w, c, best.w, idx[3]);
    }
  } else {
    float best[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) best[j] = j < np ? src[j] : 0.f;
    for (int c = 1; c < C; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < np) argmax_step(src[c * HW + j], c, best[j], idx[j]);
      }
    }
  }
}

// b[j] = the confusion bin of pixel j (label lab[j], prediction idx[j]), -1 beyond np; vec: one vector access for the labels
template <typename LT>
__device__ __forceinline__ void quad_conf_bins(const LT* lab, bool vec, int np, const int idx[4], int K, long long ignore, int b[4]) {
  LT t[4];
  if (vec) load_quad<LT, true>(lab, 4, t);
  else load_quad<LT, false>(lab, np, t);
#pragma unroll
  for (int j = 0; j < 4; ++j) b[j] = j < np ? conf_bin(t[j], idx[j], K, ignore) : -1;
}

// ---- a workgroup's u32 counts in LDS: clear, count with add_bins<true>, flush the non-zero ones into global memory ----------------
__device__ __forceinline__ void lds_counts_clear(unsigned* lds, int n) {
  for (int i = threadIdx.x; i < n; i += kThreads) lds[i] = 0u;
  __syncthreads();
}

template <typename G>
__device__ __forceinline__ void lds_counts_flush(const unsigned* lds, int n, G* g) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const unsigned v = lds[i];
    if (v) atomicAdd(g + i, (G)v);
  }
}

// The grid strides over all N * ceil(HW/4) quads, one per thread.
template <bool kVec, bool kLds, typename LT>
__global__ __launch_bounds__(kThreads) void seg_confusion_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                                int N, int C, long long HW, int K, long long ignore,
                                                                unsigned long long* __restrict__ M) {
  extern __shared__ unsigned hist[];
  const int nbins = (K + 1) * K;
  if (kLds) lds_counts_clear(hist, nbins);
  const long long nq = (HW + 3) >> 2, total = (long long)N * nq;
  for (long long base = (long long)blockIdx.x * kThreads; base < total; base += (long long)gridDim.x * kThreads) {
    const long long q = base + threadIdx.x;
    int b[4] = {-1, -1, -1, -1};
    if (q < total) {
      const long long n = q / nq, p0 = (q - n * nq) * 4;
      const int np = quad_pixels<kVec>(HW - p0);
      int idx[4];
      quad_argmax_nchw<kVec>(logits + n * C * HW + p0, C, HW, np, idx);
      quad_conf_bins(labels + n * HW + p0, kVec, np, idx, K, ignore, b);
    }
    add_bins<kLds>(b, hist, M);
  }
  if (kLds) lds_counts_flush(hist, nbins, M);
}

template <typename T>
__device__ __forceinline__ long long as_i64(const T* p, long long i) { return (long long)p[i]; }

template <typename TP, typename TT>
__global__ __launch_bounds__(kThreads) void mask_iou_stats_kernel(const TP* __restrict__ pred, const TT* __restrict__ target,
                                                                 long long HW, unsigned long long* __restrict__ out) {
  const long long n = blockIdx.y;
  const TP* P = pred + n * HW;
  const TT* T = target + n * HW;
  long long s[4] = {0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (long long)gridDim.x * kThreads) {
    const long long p = as_i64(P, i), t = as_i64(T, i);
    s[0] += p * t;
    s[1] += p > t ? p : t;
    s[2] += (1 - t) * (1 - p);
    s[3] += t;
  }
  __shared__ long long part[kThreads / 64][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    long long v = s[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    long long v = 0;
    for (int w = 0; w < kThreads / 64; ++w) v += part[w][threadIdx.x];
    atomicAdd(out + n * 4 + threadIdx.x, (unsigned long long)v);   // two's complement: a signed sum
  }
}

// #{i : th[i] <= p} on the ascending table (a NaN lands in bin 0: th <= p is false for all)
__device__ __forceinline__ int threshold_bin(const float* s_th, int pr_num, float p) {
  int lo = 0, hi = pr_num;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_th[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <typename TG>
__global__ __launch_bounds__(kThreads) void fmeasure_hist_kernel(const float* __restrict__ src, long long src_ld, const TG* __restrict__ gt,
                                                                const float* __restrict__ th, int C, int channel, long long HW,
                                                                int pr_num, unsigned* __restrict__ hist) {
  extern __shared__ unsigned smem[];
  float* s_th = (float*)smem;
  unsigned* h0 = smem + pr_num;
  unsigned* h1 = h0 + pr_num + 1;
  for (int i = threadIdx.x; i < pr_num; i += kThreads) s_th[i] = th[i];
  lds_counts_clear(h0, 2 * (pr_num + 1));   // h0 and h1; its barrier covers s_th too
  const long long n = blockIdx.y;
  const TG* G = gt + n * HW;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < HW; i += (long long)gridDim.x * kThreads) {
    float p;
    if (C == 0) {
      p = src[n * src_ld + i];
    } else {   // softmax over C, channel `channel` (trainer_cavp_avs_obj.py:343 torch.softmax(vid_pred, 1)[:, 1])
      const float* x = src + n * src_ld + i;
      float m = x[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, x[c * HW]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(x[c * HW] - m);
      p = expf(x[channel * HW] - m) / s;
    }
    const int bin = threshold_bin(s_th, pr_num, p);
    atomicAdd(h0 + bin, 1u);
    if (G[i] != (TG)0) atomicAdd(h1 + bin, 1u);
  }
  lds_counts_flush(h0, 2 * (pr_num + 1), hist + n * 2 * (pr_num + 1));
}

int chunks_for(long long work, long long per_block, int cap) {
  long long c = (work + per_block - 1) / per_block;
  return (int)(c < 1 ? 1 : (c > cap ? cap : c));
}

// ---- seg_predict: mask / probability / confusion counts straight from the low-resolution NHWC logits ----------------------------
// The full-resolution [N][C][Ho][Wo] tensor of bilinear_to_nchw_kernel is never written: a thread interpolates the C logits of
// its 4 consecutive output pixels of one row ("quad") with that kernel's taps and blend (common.h: the same f32 bits), keeps the
// running argmax (argmax_step) and, for `prob`, redoes the channel loop for the max-subtracted softmax of fmeasure_hist_kernel.
// With the x4 ratio of the model head the 4 pixels read at most 3 source columns of 2 source rows: 6 loads per channel (group)
// instead of 16; any other geometry takes the per-pixel taps.

// taps of one quad; pixels past the row's end repeat the last valid pixel (in-bounds loads, results dropped)
struct QuadTaps {
  size_t r0, r1;       // element offsets of the two source rows inside x
  int w0[4], w1[4];    // source columns of each pixel
  float w00[4], w01[4], w10[4], w11[4];
  bool shared;         // all 8 columns lie in w0[0] .. w0[0] + 2
};

template <typename T, bool kVec>
__device__ __forceinline__ void load_group(const T* p, float* v) {
  if constexpr (kVec) VecT<T>::load(p, v);
  else v[0] = Elem<T>::ld(p);
}

__device__ __forceinline__ float pick3(int s, float a, float b, float c) { return s == 0 ? a : (s == 1 ? b : c); }

// f(c, v): v[j] = interpolated logit of channel c at pixel j of the quad, for c = 0 .. C-1 in order
template <typename T, bool kVec, typename F>
__device__ __forceinline__ void quad_logits(const T* __restrict__ x, const QuadTaps& q, int C, int ldx, F&& f) {
  constexpr int VE = kVec ? VecT<T>::VE : 1;
  for (int c0 = 0; c0 < C; c0 += VE) {
    float v[4][VE];
    if (q.shared) {
      float t[2][3][VE];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int col = q.w0[0] + s <= q.w1[3] ? q.w0[0] + s : q.w1[3];   // w1[3] is the largest column of the quad
        load_group<T, kVec>(x + q.r0 + (size_t)col * ldx + c0, t[0][s]);
        load_group<T, kVec>(x + q.r1 + (size_t)col * ldx + c0, t[1][s]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s0 = q.w0[j] - q.w0[0], s1 = q.w1[j] - q.w0[0];
#pragma unroll
        for (int e = 0; e < VE; ++e)
          v[j][e] = bilinear_blend(q.w00[j], q.w01[j], q.w10[j], q.w11[j], pick3(s0, t[0][0][e], t[0][1][e], t[0][2][e]),
                                   pick3(s1, t[0][0][e], t[0][1][e], t[0][2][e]), pick3(s0, t[1][0][e], t[1][1][e], t[1][2][e]),
                                   pick3(s1, t[1][0][e], t[1][1][e], t[1][2][e]));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a[VE], b[VE], c[VE], d[VE];
        load_group<T, kVec>(x + q.r0 + (size_t)q.w0[j] * ldx + c0, a);
        load_group<T, kVec>(x + q.r0 + (size_t)q.w1[j] * ldx + c0, b);
        load_group<T, kVec>(x + q.r1 + (size_t)q.w0[j] * ldx + c0, c);
        load_group<T, kVec>(x + q.r1 + (size_t)q.w1[j] * ldx + c0, d);
#pragma unroll
        for (int e = 0; e < VE; ++e) v[j][e] = bilinear_blend(q.w00[j], q.w01[j], q.w10[j], q.w11[j], a[e], b[e], c[e], d[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (c0 + e < C) {
        const float ve[4] = {v[0][e], v[1][e], v[2][e], v[3][e]};
        f(c0 + e, ve);
      }
    }
  }
}

enum { kOutVecMask = 1, kOutVecProb = 2, kOutVecLabels = 4 };   // which per-pixel arrays take one vector access per quad

// kVec: 16-byte channel-group loads (ldx a multiple of the vector, x 16-byte aligned; the groups may run into the row's padding
// channels, never past the pitch).  kConf: 0 no counts, 1 counts privatised in LDS, 2 counts added straight into M.
// One thread = one quad; the grid strides over all N * Ho * ceil(Wo / 4) quads with a block-uniform trip count (add_bins ballots).
template <typename T, bool kVec, int kConf>
__global__ __launch_bounds__(kThreads) void seg_predict_kernel(const T* __restrict__ x, int N, int Hi, int Wi, int C, int ldx, int Ho,
                                                              int Wo, int align, unsigned char* __restrict__ mask,
                                                              float* __restrict__ prob, int channel, const void* __restrict__ labels,
                                                              int label_f32, int K, long long ignore,
                                                              unsigned long long* __restrict__ M, int out_vec) {
  extern __shared__ unsigned hist[];
  const int nbins = (K + 1) * K;
  if (kConf == 1) lds_counts_clear(hist, nbins);
  const int qpr = (Wo + 3) >> 2;
  const long long total = (long long)N * Ho * qpr;
  for (long long base = (long long)blockIdx.x * kThreads; base < total; base += (long long)gridDim.x * kThreads) {
    const long long qi = base + threadIdx.x;
    int b[4] = {-1, -1, -1, -1};
    if (qi < total) {
      int qx, ho, n;
      split_pixel(qi, qpr, Ho, qx, ho, n);
      const int wo0 = qx * 4, np = Wo - wo0 < 4 ? Wo - wo0 : 4;
      QuadTaps q;
      int h0, h1;
      float lh;
      src_index(ho, Hi, Ho, align, h0, h1, lh);
      q.r0 = ((size_t)n * Hi + h0) * Wi * ldx;
      q.r1 = ((size_t)n * Hi + h1) * Wi * ldx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float lw;
        src_index(wo0 + (j < np ? j : np - 1), Wi, Wo, align, q.w0[j], q.w1[j], lw);
        bilinear_weights(lh, lw, q.w00[j], q.w01[j], q.w10[j], q.w11[j]);
      }
      q.shared = q.w1[3] - q.w0[0] <= 2;   // columns never decrease along a row: w0[0] is the smallest, w1[3] the largest
      const float ninf = -__builtin_huge_valf();
      float best[4] = {ninf, ninf, ninf, ninf}, mx[4] = {ninf, ninf, ninf, ninf};
      int idx[4] = {0, 0, 0, 0};
      quad_logits<T, kVec>(x, q, C, ldx, [&](int c, const float* v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          argmax_step(v[j], c, best[j], idx[j]);
          mx[j] = fmaxf(mx[j], v[j]);
        }
      });
      const long long p0 = ((long long)n * Ho + ho) * Wo + wo0;
      if (mask) {
        if (out_vec & kOutVecMask) {
          *(unsigned*)(mask + p0) = (unsigned)idx[0] | ((unsigned)idx[1] << 8) | ((unsigned)idx[2] << 16) | ((unsigned)idx[3] << 24);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < np) mask[p0 + j] = (unsigned char)idx[j];
          }
        }
      }
      if (prob) {   // softmax over the C interpolated logits, channel `channel`: fmeasure_hist_kernel's arithmetic
        float s[4] = {0.f, 0.f, 0.f, 0.f}, xc[4] = {0.f, 0.f, 0.f, 0.f};
        quad_logits<T, kVec>(x, q, C, ldx, [&](int c, const float* v) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s[j] += expf(v[j] - mx[j]);
            if (c == channel) xc[j] = v[j];
          }
        });
        float pr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pr[j] = expf(xc[j] - mx[j]) / s[j];
        if (out_vec & kOutVecProb) {
          *(float4*)(prob + p0) = make_float4(pr[0], pr[1], pr[2], pr[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < np) prob[p0 + j] = pr[j];
          }
        }
      }
      if (kConf) {
        const bool vec = (out_vec & kOutVecLabels) != 0;
        if (label_f32) quad_conf_bins((const float*)labels + p0, vec, np, idx, K, ignore, b);
        else quad_conf_bins((const long long*)labels + p0, vec, np, idx, K, ignore, b);
      }
    }
    if constexpr (kConf != 0) add_bins<kConf == 1>(b, hist, M);   // kConf is a template argument: not a per-thread condition
  }
  if (kConf == 1) lds_counts_flush(hist, nbins, M);
}

// ---- clip validation: the frames of a batch of clips routed into the ALL and the multi-source (MS) matrix ------------------------
// frame_kernel: per participating frame the 256-bin label histogram and the (K+1) x K confusion counts, as u32 in per-frame scratch.
// flags_kernel: the frame's MS flag from its histogram (cleared again here), the frame counters, the bad `count` entries.
// combine_kernel: the frames' confusion counts added into ALL / MS by their flags (scratch cleared again).
constexpr int kLabelBins = 256;
constexpr int kCombineFrames = 16;   // frames per combine workgroup

// count[b] clamped to [0, T]; no count: every frame
__device__ __forceinline__ long long clip_count_raw(const void* count, int count_i64, int b) {
  return count_i64 ? ((const long long*)count)[b] : (long long)((const int*)count)[b];
}
__device__ __forceinline__ int clip_count(const void* count, int count_i64, int b, int T) {
  if (!count) return T;
  const long long c = clip_count_raw(count, count_i64, b);
  return (int)(c < 0 ? 0 : (c > T ? T : c));
}

// grid (chunks, B*T): a workgroup belongs to one frame.  One thread = 4 consecutive pixels; block-uniform trip count (add_bins
// ballots).  LDS: [256] label histogram, then (kLds) the frame's (K+1)*K confusion counts.  Every index is guarded before use: the
// histogram bin by v < 256 (v < 0 takes `ignore`, which the host checks to be in [0, 256)), the confusion bin by p < K.
template <bool kMask, bool kVec, bool kLds>
__global__ __launch_bounds__(kThreads) void clipval_frame_kernel(const void* __restrict__ pred, const long long* __restrict__ labels,
                                                                const void* __restrict__ count, int count_i64, int T, int C,
                                                                long long HW, int K, int ignore, unsigned* __restrict__ hist,
                                                                unsigned* __restrict__ conf, unsigned long long* __restrict__ state) {
  extern __shared__ unsigned lds[];
  const int n = blockIdx.y, b = n / T, t = n - b * T;
  if (t >= clip_count(count, count_i64, b, T)) return;   // workgroup-uniform: the frame is not read
  const int nbins = (K + 1) * K;
  unsigned* lconf = lds + kLabelBins;
  lds_counts_clear(lds, kLabelBins + (kLds ? nbins : 0));
  unsigned* gconf = conf + (size_t)n * nbins;
  const long long* lab_n = labels + (long long)n * HW;
  const long long nq = (HW + 3) >> 2;
  unsigned bad_label = 0, bad_mask = 0;
  for (long long base = (long long)blockIdx.x * kThreads; base < nq; base += (long long)gridDim.x * kThreads) {
    const long long q = base + threadIdx.x;
    int hb[4] = {-1, -1, -1, -1}, cb[4] = {-1, -1, -1, -1};
    if (q < nq) {
      const long long p0 = q * 4;
      const int np = quad_pixels<kVec>(HW - p0);
      long long tv[4];
      load_quad<long long, kVec>(lab_n + p0, np, tv);
      int p[4];
      if (kMask) {
        unsigned char m[4];
        load_quad<unsigned char, kVec>((const unsigned char*)pred + (long long)n * HW + p0, np, m);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = m[j];
      } else {
        quad_argmax_nchw<kVec>((const float*)pred + (long long)n * C * HW + p0, C, HW, np, p);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= np) continue;
        const long long v = tv[j];
        if (v >= kLabelBins) { ++bad_label; continue; }
        if (kMask && p[j] >= K) { ++bad_mask; continue; }
        hb[j] = v < 0 ? ignore : (int)v;
        if (v >= 0 && v != ignore) cb[j] = (v < K ? (int)v : K) * K + p[j];
      }
    }
    add_bins<true>(hb, lds, (unsigned*)nullptr);
    add_bins<kLds>(cb, lconf, gconf);
  }
  if (bad_label) atomicAdd(state, (unsigned long long)bad_label);
  if (bad_mask) atomicAdd(state + 1, (unsigned long long)bad_mask);
  lds_counts_flush(lds, kLabelBins, hist + (size_t)n * kLabelBins);
  if (kLds) lds_counts_flush(lconf, nbins, gconf);
}

// grid B*T, 256 threads = the 256 histogram bins of one frame.  flags[n]: 0 = takes no part, 1 = ALL, 3 = ALL and MS.
__global__ __launch_bounds__(kLabelBins) void clipval_flags_kernel(unsigned* __restrict__ hist, unsigned* __restrict__ flags,
                                                                  const void* __restrict__ count, int count_i64, int T,
                                                                  unsigned min_count, int min_values,
                                                                  unsigned long long* __restrict__ frames,
                                                                  unsigned long long* __restrict__ state) {
  __shared__ int part[kLabelBins / 64];
  const int n = blockIdx.x, b = n / T, t = n - b * T;
  if (t == 0 && threadIdx.x == 0 && count) {
    const long long c = clip_count_raw(count, count_i64, b);
    if (c < 0 || c > T) atomicAdd(state + 2, 1ull);
  }
  if (t >= clip_count(count, count_i64, b, T)) {   // workgroup-uniform
    if (threadIdx.x == 0) flags[n] = 0u;
    return;
  }
  unsigned* h = hist + (size_t)n * kLabelBins + threadIdx.x;
  const unsigned v = *h;
  if (v) *h = 0u;
  const int q = __popcll(__ballot(v > min_count));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    int values = 0;
#pragma unroll
    for (int w = 0; w < kLabelBins / 64; ++w) values += part[w];
    const bool ms = values > min_values;
    flags[n] = ms ? 3u : 1u;
    atomicAdd(frames, 1ull);
    if (ms) atomicAdd(frames + 1, 1ull);
  }
}

// grid (ceil(nbins / 256), ceil(N / kCombineFrames)): one thread = one bin of kCombineFrames frames
__global__ __launch_bounds__(kThreads) void clipval_combine_kernel(unsigned* __restrict__ conf, const unsigned* __restrict__ flags, int N,
                                                                  int nbins, unsigned long long* __restrict__ counts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nbins) return;
  const int n0 = blockIdx.y * kCombineFrames;
  unsigned v[kCombineFrames], f[kCombineFrames];
#pragma unroll
  for (int k = 0; k < kCombineFrames; ++k) {
    f[k] = n0 + k < N ? flags[n0 + k] : 0u;
    v[k] = f[k] ? conf[(size_t)(n0 + k) * nbins + i] : 0u;
  }
  unsigned long long all = 0, ms = 0;
#pragma unroll
  for (int k = 0; k < kCombineFrames; ++k) {
    if (v[k]) {
      conf[(size_t)(n0 + k) * nbins + i] = 0u;
      all += v[k];
      if (f[k] & 2u) ms += v[k];
    }
  }
  if (all) atomicAdd(counts + i, all);
  if (ms) atomicAdd(counts + nbins + i, ms);
}

// ---- video validation: per-video J (mask IoU) and F (best F-measure) of the AVSBench object sets ----------------------------------
// frame_kernel: per participating frame, from one read of the prediction, the four mask_iou_stats sums, the two fmeasure_hist
//               histograms (per-frame scratch) and the seg_confusion counts (straight into the global matrix).
// combine_kernel: one workgroup per video: the float32 tail of mask_iou and Eval_Fmeasure, J and F into the video's slot, the
//               scratch cleared again, the slot base advanced by the last workgroup to finish.
constexpr int kSoftmaxRegC = 4;   // logits of at most this many channels are held in registers between argmax and softmax
enum { kVvBadLabel = 0, kVvBadMask = 1, kVvBadCount = 2, kVvDropped = 3, kVvVideos = 4, kVvTicket = 5 };   // state words

// idx[j]: quad_argmax_nchw's argmax; pr[j]: fmeasure_hist_kernel's softmax of channel `channel` (max-subtracted, the channels
// summed in ascending order, IEEE division) of pixel j of the quad at src.
template <bool kVec>
__device__ __forceinline__ void quad_argmax_softmax_nchw(const float* src, int C, long long HW, int np, int channel, int idx[4],
                                                         float pr[4]) {
  if (C <= kSoftmaxRegC) {
    float v[kSoftmaxRegC][4];
#pragma unroll
    for (int c = 0; c < kSoftmaxRegC; ++c) {
      if (c < C) load_quad<float, kVec>(src + c * HW, np, v[c]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float best = v[0][j], m = v[0][j];
      idx[j] = 0;
#pragma unroll
      for (int c = 1; c < kSoftmaxRegC; ++c) {
        if (c < C) {
          argmax_step(v[c][j], c, best, idx[j]);
          m = fmaxf(m, v[c][j]);
        }
      }
      float s = 0.f, xc = 0.f;
#pragma unroll
      for (int c = 0; c < kSoftmaxRegC; ++c) {
        if (c < C) {
          s += expf(v[c][j] - m);
          if (c == channel) xc = v[c][j];
        }
      }
      pr[j] = expf(xc - m) / s;
    }
  } else {
    quad_argmax_nchw<kVec>(src, C, HW, np, idx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pr[j] = 0.f;
      if (j < np) {
        const float* x = src + j;
        float m = x[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, x[c * HW]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(x[c * HW] - m);
        pr[j] = expf(x[channel * HW] - m) / s;
      }
    }
  }
}

// grid (chunks, B*T): a workgroup belongs to one frame.  One thread = 4 consecutive pixels; block-uniform trip count (add_bins
// ballots).  LDS: [pr_num] thresholds, [2][pr_num+1] histograms, then (kLds) the workgroup's (K+1)*K confusion counts.  The
// histogram bin is bounded by the search (<= pr_num), the confusion bin by p < K (a mask byte >= K sets none).
template <bool kMask, bool kVec, bool kLds>
__global__ __launch_bounds__(kThreads) void videoval_frame_kernel(const void* __restrict__ pred, const float* __restrict__ prob,
                                                                 const long long* __restrict__ labels, const void* __restrict__ count,
                                                                 int count_i64, int T, int C, int channel, long long HW, int K,
                                                                 long long ignore, const float* __restrict__ th, int pr_num,
                                                                 unsigned long long* __restrict__ stats, unsigned* __restrict__ hist,
                                                                 unsigned long long* __restrict__ M, unsigned long long* __restrict__ state) {
  extern __shared__ unsigned lds[];
  const int n = blockIdx.y, b = n / T, t = n - b * T;
  if (t >= clip_count(count, count_i64, b, T)) return;   // workgroup-uniform: the frame is not read
  const int nbins = (K + 1) * K, nh = 2 * (pr_num + 1);
  float* s_th = (float*)lds;
  unsigned* h0 = lds + pr_num;
  unsigned* h1 = h0 + pr_num + 1;
  unsigned* lconf = h0 + nh;
  for (int i = threadIdx.x; i < pr_num; i += kThreads) s_th[i] = th[i];
  lds_counts_clear(h0, nh + (kLds ? nbins : 0));   // its barrier covers s_th too
  const long long* lab_n = labels + (long long)n * HW;
  const long long nq = (HW + 3) >> 2;
  long long s[4] = {0, 0, 0, 0};
  unsigned bad_label = 0, bad_mask = 0;
  for (long long base = (long long)blockIdx.x * kThreads; base < nq; base += (long long)gridDim.x * kThreads) {
    const long long q = base + threadIdx.x;
    int cb[4] = {-1, -1, -1, -1};
    if (q < nq) {
      const long long p0 = q * 4;
      const int np = quad_pixels<kVec>(HW - p0);
      long long tv[4];
      load_quad<long long, kVec>(lab_n + p0, np, tv);
      int p[4];
      float pr[4];
      if (kMask) {
        unsigned char m[4];
        load_quad<unsigned char, kVec>((const unsigned char*)pred + (long long)n * HW + p0, np, m);
        load_quad<float, kVec>(prob + (long long)n * HW + p0, np, pr);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = m[j];
      } else {
        quad_argmax_softmax_nchw<kVec>((const float*)pred + (long long)n * C * HW + p0, C, HW, np, channel, p, pr);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= np) continue;
        const long long v = tv[j], pj = p[j];
        const int bin = threshold_bin(s_th, pr_num, pr[j]);
        atomicAdd(h0 + bin, 1u);
        if (v != 0) atomicAdd(h1 + bin, 1u);
        s[0] += pj * v;
        s[1] += pj > v ? pj : v;
        s[2] += (1 - v) * (1 - pj);
        s[3] += v;
        if (v != 0 && v != 1 && v != ignore) ++bad_label;
        if (kMask && p[j] >= K) ++bad_mask;
        else cb[j] = conf_bin(v, p[j], K, ignore);
      }
    }
    add_bins<kLds>(cb, lconf, M);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    long long v = s[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(stats + (size_t)n * 4 + k, (unsigned long long)v);   // two's complement: a signed sum
  }
  if (bad_label) atomicAdd(state + kVvBadLabel, (unsigned long long)bad_label);
  if (bad_mask) atomicAdd(state + kVvBadMask, (unsigned long long)bad_mask);
  lds_counts_flush(h0, nh, hist + (size_t)n * nh);
  if (kLds) lds_counts_flush(lconf, nbins, M);
}

// sum over the workgroup of two ints per thread; part: [2][kThreads / 64] in LDS
__device__ __forceinline__ void block_sum2(int& a, int& b, int (*part)[kThreads / 64]) {
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = a; part[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  a = b = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) { a += part[0][w]; b += part[1][w]; }
}

constexpr int kWaves = kThreads / 64;

// LDS words of a combine workgroup: a [2][pr_num+1] histogram per wave, kWaves + 1 rows of [pr_num] floats, [kThreads] floats
__host__ __device__ constexpr size_t videoval_combine_words(int pr_num) {
  return (size_t)kWaves * 2 * (pr_num + 1) + (size_t)(kWaves + 1) * pr_num + kThreads;
}

// grid B: one workgroup = one video.  The frames are taken kWaves at a time, one wave per frame: the wave turns its frame's two
// histograms into suffix sums in LDS (a lane sums its run of bins, the lane totals are scanned with shuffles) and writes f of every
// threshold; then the workgroup adds the group's f rows to the running sums in ascending frame order.  Every float step is one
// IEEE operation (__f*_rn: the build contracts a * b + c).
__global__ __launch_bounds__(kThreads) void videoval_combine_kernel(unsigned long long* __restrict__ stats, unsigned* __restrict__ hist,
                                                                   const void* __restrict__ count, int count_i64, int B, int T,
                                                                   long long HW, int pr_num, int max_videos, float* __restrict__ J,
                                                                   float* __restrict__ F, unsigned long long* __restrict__ state) {
  extern __shared__ unsigned lds[];
  __shared__ int part[2][kWaves];
  __shared__ float wave_max[kWaves];
  __shared__ int valid[kWaves];
  const int nb = pr_num + 1, nh = 2 * nb;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned* cnts = lds + (size_t)wave * nh;         // this wave's frame: [2][nb] counts, then their suffix sums
  float* fbuf = (float*)(lds + (size_t)kWaves * nh);   // [kWaves][pr_num]: f of the group's frames
  float* acc = fbuf + (size_t)kWaves * pr_num;      // [pr_num]: the sums of f over the frames kept
  float* iou = acc + pr_num;                        // [kThreads]: overlap / union of a run of frames
  const int b = blockIdx.x;
  const int cnt = clip_count(count, count_i64, b, T);
  // videos with frames in front of this one, and in the whole call
  int before = b, videos = B;
  if (count) {
    before = videos = 0;
    for (int i = threadIdx.x; i < B; i += kThreads) {
      const int has = clip_count(count, count_i64, i, T) > 0 ? 1 : 0;
      videos += has;
      if (i < b) before += has;
    }
    block_sum2(before, videos, part);
  }
  if (cnt > 0) {   // workgroup-uniform
    // J: the frames' quotients side by side, then added by one thread in ascending order
    float sum = 0.f;
    for (int t0 = 0; t0 < cnt; t0 += kThreads) {
      const int t = t0 + threadIdx.x;
      if (t < cnt) {
        const unsigned long long* s = stats + ((size_t)b * T + t) * 4;
        long long overlap = (long long)s[0], uni = (long long)s[1];
        if (s[3] == 0ull) { overlap = (long long)s[2]; uni = HW; }   // mask_iou's empty target: the background overlap over all pixels
        iou[threadIdx.x] = __fdiv_rn((float)overlap, __fadd_rn((float)uni, 1e-7f));
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = cnt - t0 < kThreads ? cnt - t0 : kThreads;
        for (int k = 0; k < n; ++k) sum = __fadd_rn(sum, iou[k]);
      }
      __syncthreads();
    }
    // F
    for (int i = threadIdx.x; i < pr_num; i += kThreads) acc[i] = 0.f;
    int kept = 0;
    const int run = (nb + 63) >> 6;   // bins per lane
    for (int t0 = 0; t0 < cnt; t0 += kWaves) {
      const bool mine = t0 + wave < cnt;   // wave-uniform
      if (mine) {
        const unsigned* h = hist + ((size_t)b * T + t0 + wave) * nh;
        for (int i = lane; i < nh; i += 64) cnts[i] = h[i];
      }
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {   // cnts[a][k] = sum over k' >= k
          unsigned* c = cnts + a * nb;
          const int lo = lane * run < nb ? lane * run : nb, hi = lo + run < nb ? lo + run : nb;
          unsigned own = 0;
          for (int k = lo; k < hi; ++k) own += c[k];
          unsigned suf = own;   // the total of this lane and the lanes above it
          for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_down(suf, o, 64);
            if (lane + o < 64) suf += v;
          }
          unsigned above = suf - own;
          for (int k = hi - 1; k >= lo; --k) {
            above += c[k];
            c[k] = above;
          }
        }
      }
      __syncthreads();
      if (mine) {
        const unsigned* all = cnts;
        const unsigned* pos = cnts + nb;
        if (lane == 0) valid[wave] = pos[0] != 0u;   // an all-zero gt: the frame is skipped
        if (pos[0] != 0u) {
          const float ysum = __fadd_rn((float)pos[0], 1e-20f);
          for (int i = lane; i < pr_num; i += 64) {
            const float tp = (float)pos[i + 1];
            const float prec = __fdiv_rn(tp, __fadd_rn((float)all[i + 1], 1e-20f));
            const float recall = __fdiv_rn(tp, ysum);
            float f = __fdiv_rn(__fmul_rn(__fmul_rn((float)(1.0 + 0.3), prec), recall), __fadd_rn(__fmul_rn(0.3f, prec), recall));
            if (f != f) f = 0.f;
            fbuf[(size_t)wave * pr_num + i] = f;
          }
        }
      }
      __syncthreads();
      const int frames = cnt - t0 < kWaves ? cnt - t0 : kWaves;
      for (int w = 0; w < frames; ++w) {   // ascending t
        if (!valid[w]) continue;           // workgroup-uniform
        ++kept;
        for (int i = threadIdx.x; i < pr_num; i += kThreads) acc[i] = __fadd_rn(acc[i], fbuf[(size_t)w * pr_num + i]);   // acc[i] is this thread's
      }
      __syncthreads();   // fbuf, valid and cnts are free again
    }
    float best = 0.f;   // every score is >= 0
    for (int i = threadIdx.x; i < pr_num; i += kThreads) {
      const float score = kept > 0 ? __fdiv_rn(acc[i], (float)kept) : 0.f;
      best = fmaxf(best, score);
    }
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    if (lane == 0) wave_max[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < kWaves; ++w) best = fmaxf(best, wave_max[w]);
      // the slot base is only advanced by the last workgroup of this launch, after every workgroup has read it
      const unsigned long long slot = atomicAdd(state + kVvVideos, 0ull) + (unsigned long long)before;
      if (slot < (unsigned long long)max_videos) {
        J[slot] = __fdiv_rn(sum, (float)cnt);
        F[slot] = best;
      } else {
        atomicAdd(state + kVvDropped, 1ull);
      }
    }
    // every read of this video's scratch lies before the last barrier above: clear it
    unsigned long long* s = stats + (size_t)b * T * 4;
    for (int i = threadIdx.x; i < cnt * 4; i += kThreads) s[i] = 0ull;
    unsigned* h = hist + (size_t)b * T * nh;
    for (long long i = threadIdx.x; i < (long long)cnt * nh; i += kThreads) h[i] = 0u;
  }
  if (threadIdx.x == 0) {
    if (count) {
      const long long c = clip_count_raw(count, count_i64, b);
      if (c < 0 || c > T) atomicAdd(state + kVvBadCount, 1ull);
    }
    __threadfence();
    if (atomicAdd(state + kVvTicket, 1ull) == (unsigned long long)(B - 1)) {   // the last workgroup of the launch
      atomicAdd(state + kVvVideos, (unsigned long long)videos);
      atomicExch(state + kVvTicket, 0ull);
    }
  }
}

// ---- semantic validation: per-frame, per-class IoU and F-score of the AVSBench-semantic metric (utils/avsbench_metrics.py) -------
// frame_kernel:   per participating frame, from one read of the prediction, the three class-area vectors inter | pred | lab and the
//                 four binary-IoU sums as u32 in per-frame scratch [3K + 4].
// combine_kernel: one thread per class walks the call's frames in ascending order (float32, one IEEE operation at a time) and adds
//                 the call's partial to the running accumulators; the last workgroup to finish turns the per-frame IoUs the class
//                 threads left in the scratch into frame_miou, finishes the binary IoU and leaves the scratch zero.
enum { kSvBadMask = 0, kSvBadCount = 1, kSvFrames = 2, kSvTicket = 3 };   // state words
constexpr int kSemvalQuads = 2;    // quads per thread of a frame workgroup
constexpr int kSemvalChunk = 16;   // frames a class thread loads side by side
constexpr int kSemvalCombineThreads = 1024;   // 16 waves: the last workgroup takes 16 frames at a time
constexpr int kSemvalCombineWaves = kSemvalCombineThreads / 64;

// grid (chunks, B*T): a workgroup belongs to one frame.  One thread = 4 consecutive pixels; block-uniform trip count (add_bins
// ballots).  LDS: [K] inter, [K] pred, [K] lab, [4] binary sums.  Every index is guarded before use: a prediction by p < K (logits
// have C == K channels, a mask byte >= K sets no class bin), a label by 0 <= v < K.
template <bool kMask, bool kVec>
__global__ __launch_bounds__(kThreads) void semval_frame_kernel(const void* __restrict__ pred, const long long* __restrict__ labels,
                                                               const void* __restrict__ count, int count_i64, int T, long long HW,
                                                               int K, unsigned* __restrict__ scratch,
                                                               unsigned long long* __restrict__ state) {
  extern __shared__ unsigned lds[];
  const int n = blockIdx.y, b = n / T, t = n - b * T;
  if (t >= clip_count(count, count_i64, b, T)) return;   // workgroup-uniform: the frame is not read
  const int words = 3 * K + 4;
  lds_counts_clear(lds, words);
  const long long* lab_n = labels + (long long)n * HW;
  const long long nq = (HW + 3) >> 2;
  unsigned bad_mask = 0;
  int bin[4] = {0, 0, 0, 0};   // #(P and G), #(P or G), #(neither), #G with P = (p != 0), G = (v != 0)
  for (long long base = (long long)blockIdx.x * kThreads; base < nq; base += (long long)gridDim.x * kThreads) {
    const long long q = base + threadIdx.x;
    int bi[4] = {-1, -1, -1, -1}, bp[4] = {-1, -1, -1, -1}, bl[4] = {-1, -1, -1, -1};
    if (q < nq) {
      const long long p0 = q * 4;
      const int np = quad_pixels<kVec>(HW - p0);
      long long tv[4];
      load_quad<long long, kVec>(lab_n + p0, np, tv);
      int p[4];
      if (kMask) {
        unsigned char m[4];
        load_quad<unsigned char, kVec>((const unsigned char*)pred + (long long)n * HW + p0, np, m);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = m[j];
      } else {
        quad_argmax_nchw<kVec>((const float*)pred + (long long)n * K * HW + p0, K, HW, np, p);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= np) continue;
        const long long v = tv[j];
        const bool P = p[j] != 0, G = v != 0;
        bin[0] += P && G;
        bin[1] += P || G;
        bin[2] += !P && !G;
        bin[3] += G;
        if (kMask && p[j] >= K) { ++bad_mask; continue; }
        if (v < 0) continue;            // counts in none of the three areas
        bp[j] = K + p[j];               // a label >= K (the ignore value) still counts the prediction: histc drops only the label
        if (v < K) {
          bl[j] = 2 * K + (int)v;
          if (v == p[j]) bi[j] = p[j];
        }
      }
    }
    add_bins<true>(bi, lds, (unsigned*)nullptr);
    add_bins<true>(bp, lds, (unsigned*)nullptr);
    add_bins<true>(bl, lds, (unsigned*)nullptr);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int v = bin[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(lds + 3 * K + k, (unsigned)v);
  }
  if (bad_mask) atomicAdd(state + kSvBadMask, (unsigned long long)bad_mask);
  lds_counts_flush(lds, words, scratch + (size_t)n * words);   // its barrier covers the binary sums
}

// a word another workgroup of this launch has written: read at the device's level of coherence, never from this CU's cache
__device__ __forceinline__ unsigned load_device_scope(const unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid ceil(K / 1024): one thread = one class.  acc: f32 [3K + 1] ious | fscores | cls_count | binary sum (running); last: f32
// [3K + 1 + 2 * max_frames] the same of this call, then frame_miou and the frames' binary IoU.  Every float step is one IEEE
// operation (__f*_rn: the build contracts a * b + c).
__global__ __launch_bounds__(kSemvalCombineThreads) void semval_combine_kernel(unsigned* __restrict__ scratch, const void* __restrict__ count,
                                                                 int count_i64, int B, int T, long long HW, int K, int max_frames,
                                                                 float* __restrict__ acc, float* __restrict__ last,
                                                                 unsigned long long* __restrict__ state) {
  __shared__ int is_last;
  __shared__ float biou[kSemvalCombineThreads];
  const int N = B * T, words = 3 * K + 4;
  const int c = blockIdx.x * kSemvalCombineThreads + threadIdx.x;
  if (c < K) {
    float s_iou = 0.f, s_f = 0.f, s_hit = 0.f;
    for (int n0 = 0; n0 < N; n0 += kSemvalChunk) {
      unsigned a[kSemvalChunk][3];
      bool on[kSemvalChunk];
#pragma unroll
      for (int k = 0; k < kSemvalChunk; ++k) {
        const int n = n0 + k, b = n / T;
        on[k] = n < N && n - b * T < clip_count(count, count_i64, b, T);
        if (on[k]) {
          const unsigned* s = scratch + (size_t)n * words + c;
          a[k][0] = s[0]; a[k][1] = s[K]; a[k][2] = s[2 * K];
        }
      }
#pragma unroll
      for (int k = 0; k < kSemvalChunk; ++k) {   // ascending frames
        if (!on[k]) continue;
        const float inter = (float)a[k][0], pred = (float)a[k][1], lab = (float)a[k][2];
        const float uni = __fsub_rn(__fadd_rn(pred, lab), inter);
        const float iou = __fdiv_rn(inter, __fadd_rn(2.220446049250313e-16f, uni));
        const float prec = __fdiv_rn(inter, pred), recall = __fdiv_rn(inter, lab);
        float f = __fdiv_rn(__fmul_rn(__fmul_rn(1.3f, prec), recall), __fadd_rn(__fmul_rn(0.3f, prec), recall));
        if (f != f) f = 0.f;
        s_iou = __fadd_rn(s_iou, iou);
        s_f = __fadd_rn(s_f, f);
        if (uni != 0.f) s_hit = __fadd_rn(s_hit, 1.f);
        unsigned* s = scratch + (size_t)(n0 + k) * words + c;
        if (a[k][0]) s[0] = __float_as_uint(iou);   // the frame's IoU (non-zero iff inter is), for the last workgroup
        if (a[k][1]) s[K] = 0u;
        if (a[k][2]) s[2 * K] = 0u;
      }
    }
    last[c] = s_iou;
    last[K + c] = s_f;
    last[2 * K + c] = s_hit;
    acc[c] = __fadd_rn(acc[c], s_iou);
    acc[K + c] = __fadd_rn(acc[K + c], s_f);
    acc[2 * K + c] = __fadd_rn(acc[2 * K + c], s_hit);
  }
  if (gridDim.x == 1) {   // K <= 1024: this workgroup wrote every IoU itself, a barrier orders them; no ticket, no device-wide fence
    __syncthreads();
  } else {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(state + kSvTicket, 1ull) == (unsigned long long)(gridDim.x - 1);
    __syncthreads();
    if (!is_last) return;   // workgroup-uniform
    __threadfence();        // every class thread of the launch has left its IoUs in the scratch
    if (threadIdx.x == 0) atomicExch(state + kSvTicket, 0ull);
  }

  float* frame_miou = last + 3 * K + 1;
  float* frame_biou = frame_miou + max_frames;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // frame_miou: one wave per frame; a lane loads its class, the wave adds the classes in ascending order (every lane the same sum)
  for (int n = wave; n < N; n += kSemvalCombineWaves) {
    const int b = n / T;
    if (n - b * T >= clip_count(count, count_i64, b, T)) {   // wave-uniform
      if (lane == 0) frame_miou[n] = -1.f;
      continue;
    }
    unsigned* s = scratch + (size_t)n * words;
    float sum = 0.f;
    int nz = 0;
    // the first two loads are in flight together (K <= 128 needs no more); a lane beyond K holds 0, which changes neither result
    unsigned ahead = 64 + lane < K ? load_device_scope(s + 64 + lane) : 0u;
    for (int c0 = 0; c0 < K; c0 += 64) {
      const unsigned mine = c0 == 64 ? ahead : (c0 + lane < K ? load_device_scope(s + c0 + lane) : 0u);
      if (mine) s[c0 + lane] = 0u;
#pragma unroll
      for (int i = 0; i < 64; ++i) {   // lane i's value through a scalar register: no LDS traffic
        const float v = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)mine, i));
        sum = __fadd_rn(sum, v);
        nz += v != 0.f;
      }
    }
    if (lane == 0) frame_miou[n] = __fdiv_rn(sum, (float)nz);   // no class with a non-zero IoU: 0 / 0, the reference's NaN
  }
  // binary IoU: the frames' quotients side by side, then added by one thread in ascending order
  float bsum = 0.f;
  int frames = 0;
  for (int n0 = 0; n0 < N; n0 += kSemvalCombineThreads) {
    const int n = n0 + threadIdx.x;
    float v = -1.f;   // takes no part (a quotient is >= 0)
    if (n < N) {
      const int b = n / T;
      if (n - b * T < clip_count(count, count_i64, b, T)) {
        unsigned* s = scratch + (size_t)n * words + 3 * K;
        unsigned inter = s[0], uni = s[1];
        if (s[3] == 0u) { inter = s[2]; uni = (unsigned)HW; }   // an empty target: the background overlap over all pixels
        v = __fdiv_rn((float)inter, __fadd_rn((float)uni, 1e-7f));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (s[k]) s[k] = 0u;
        }
      }
      frame_biou[n] = v;
    }
    biou[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = N - n0 < kSemvalCombineThreads ? N - n0 : kSemvalCombineThreads;
      for (int k = 0; k < m; ++k) {
        if (biou[k] >= 0.f) { bsum = __fadd_rn(bsum, biou[k]); ++frames; }
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    last[3 * K] = bsum;
    acc[3 * K] = __fadd_rn(acc[3 * K], bsum);
    if (frames) atomicAdd(state + kSvFrames, (unsigned long long)frames);
  }
  if (count) {
    unsigned bad = 0;
    for (int b = threadIdx.x; b < B; b += kSemvalCombineThreads) {
      const long long cb = clip_count_raw(count, count_i64, b);
      bad += cb < 0 || cb > T;
    }
    if (bad) atomicAdd(state + kSvBadCount, (unsigned long long)bad);
  }
}

// ---- host side: the checks the entry points share, run-time arguments -> template arguments -------------------------------------
bool label_ok(int code) { return code == CAVP_I64 || code == CAVP_F32; }
bool classes_ok(int K, int C) { return K >= C && K <= CAVP_METRICS_MAX_CLASSES; }
// p (may be null) is aligned for int64 elements (wide) or for 4-byte ones
bool aligned_for(const void* p, bool wide) { return ((uintptr_t)p & (wide ? 7 : 3)) == 0; }
bool label_aligned(const void* p, int code) { return aligned_for(p, code == CAVP_I64); }
// the (K+1) x K counts of one workgroup fit the u32 LDS histogram; otherwise the kernels add straight into global memory
bool counts_fit_lds(int K) { return (K + 1) * K <= kLdsBins; }

// f(LT{}) with LT = long long / float for a label dtype code the caller has validated (label_ok)
template <typename F>
void dispatch_label(int code, F&& f) {
  if (code == CAVP_I64)
    f((long long)0);
  else
    f(0.f);
}

// seg_predict_kernel's kConf: 0 no counts, 1 counts in LDS, 2 counts straight into M
template <typename F>
void dispatch_conf(int conf, F&& f) {
  if (conf == 0)
    f(std::integral_constant<int, 0>{});
  else if (conf == 1)
    f(std::integral_constant<int, 1>{});
  else
    f(std::integral_constant<int, 2>{});
}

// K = 127: 64 KiB of counts + the 1 KiB label histogram, past the 64 KiB default; once per instantiation
template <bool kMask, bool kVec, bool kLds>
void clipval_frame_allow_lds() {
  static const hipError_t once = hipFuncSetAttribute((const void*)clipval_frame_kernel<kMask, kVec, kLds>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (kLdsBins + kLabelBins) * (int)sizeof(unsigned));
  (void)once;
}

}  // namespace

extern "C" int cavp_seg_confusion_nchw(const float* logits, const void* labels, int32_t label_dtype, int32_t N, int32_t C, int64_t HW,
                                       int32_t K, int64_t ignore, uint64_t* M, void* stream) {
  if (!logits || !labels || !M || N <= 0 || C <= 0 || HW <= 0 || K <= 0) return CAVP_ERR_BAD_ARG;
  if (!classes_ok(K, C)) return CAVP_ERR_UNSUPPORTED;
  if (!label_ok(label_dtype)) return CAVP_ERR_UNSUPPORTED;
  if (!label_aligned(labels, label_dtype) || ((uintptr_t)M & 7) || ((uintptr_t)logits & 3)) return CAVP_ERR_ALIGN;
  const bool vec = (HW & 3) == 0 && al16(logits) && al16(labels);
  const bool lds = counts_fit_lds(K);
  const long long quads = (long long)N * ((HW + 3) >> 2);
  // one quad per thread for B=32 at 224^2 (1568 workgroups, all resident); each workgroup flushes its non-zero LDS bins once
  const int grid = chunks_for(quads, kThreads, lds ? 2048 : 4096);
  const size_t shm = lds ? (size_t)(K + 1) * K * sizeof(unsigned) : 0;
  hipStream_t s = (hipStream_t)stream;
  dispatch_label(label_dtype, [&](auto t) { using LT = decltype(t);
    cavp_dispatch_bool(vec, [&](auto v) { cavp_dispatch_bool(lds, [&](auto l) {
      seg_confusion_kernel<decltype(v)::value, decltype(l)::value, LT><<<grid, kThreads, shm, s>>>(
          logits, (const LT*)labels, N, C, HW, K, ignore, (unsigned long long*)M); }); }); });
  CHECK_LAUNCH();
}

extern "C" int cavp_seg_predict_nhwc(int32_t dtype, const void* x, int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t ldx, int32_t Ho,
                                     int32_t Wo, int32_t align_corners, uint8_t* mask, float* prob, int32_t channel, const void* labels,
                                     int32_t label_dtype, int32_t K, int64_t ignore, uint64_t* M, void* stream) {
  if (!x || N <= 0 || Hi <= 0 || Wi <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || ldx < C) return CAVP_ERR_BAD_ARG;
  if ((!mask && !prob && !M) || (!labels != !M)) return CAVP_ERR_BAD_ARG;
  if (prob && (channel < 0 || channel >= C)) return CAVP_ERR_BAD_ARG;
  if (M && K <= 0) return CAVP_ERR_BAD_ARG;
  if (!dt_ok(dtype)) return CAVP_ERR_UNSUPPORTED;
  if (mask && C > 256) return CAVP_ERR_UNSUPPORTED;
  if (M && (!classes_ok(K, C) || !label_ok(label_dtype))) return CAVP_ERR_UNSUPPORTED;
  // without M there are no labels (null: aligned for any dtype code)
  if (((uintptr_t)x & (dtype == CAVP_F32 ? 3 : 1)) || ((uintptr_t)prob & 3) || !label_aligned(labels, label_dtype) || ((uintptr_t)M & 7))
    return CAVP_ERR_ALIGN;
  const bool vec = ldx % dt_ve(dtype) == 0 && al16(x);
  const int conf = !M ? 0 : (counts_fit_lds(K) ? 1 : 2);
  int out_vec = 0;
  if ((Wo & 3) == 0) out_vec = (((uintptr_t)mask & 3) ? 0 : kOutVecMask) | (al16(prob) ? kOutVecProb : 0) | (al16(labels) ? kOutVecLabels : 0);
  const long long quads = (long long)N * Ho * ((Wo + 3) >> 2);
  const int grid = chunks_for(quads, kThreads, conf == 2 ? 4096 : 2048);
  const size_t shm = conf == 1 ? (size_t)(K + 1) * K * sizeof(unsigned) : 0;
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
    cavp_dispatch_bool(vec, [&](auto v) { dispatch_conf(conf, [&](auto cf) {
      seg_predict_kernel<T, decltype(v)::value, decltype(cf)::value><<<grid, kThreads, shm, s>>>(
          (const T*)x, N, Hi, Wi, C, ldx, Ho, Wo, align_corners, mask, prob, channel, labels, label_dtype == CAVP_F32, K, ignore,
          (unsigned long long*)M, out_vec); }); }); });
  CHECK_LAUNCH();
}

extern "C" int cavp_mask_iou_stats(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t N,
                                   int64_t HW, int64_t* out, void* stream) {
  if (!pred || !target || !out || N <= 0 || HW <= 0) return CAVP_ERR_BAD_ARG;
  if (!label_ok(pred_dtype) || !label_ok(target_dtype)) return CAVP_ERR_UNSUPPORTED;
  if (!label_aligned(pred, pred_dtype) || !label_aligned(target, target_dtype) || ((uintptr_t)out & 7)) return CAVP_ERR_ALIGN;
  const dim3 grid(chunks_for(HW, 4 * kThreads, 256), N);
  hipStream_t s = (hipStream_t)stream;
  dispatch_label(pred_dtype, [&](auto p) { using TP = decltype(p);
    dispatch_label(target_dtype, [&](auto t) { using TT = decltype(t);
      mask_iou_stats_kernel<TP, TT><<<grid, kThreads, 0, s>>>((const TP*)pred, (const TT*)target, HW, (unsigned long long*)out); }); });
  CHECK_LAUNCH();
}

extern "C" int cavp_fmeasure_hist(const float* src, int64_t src_image_stride, const void* gt, int32_t gt_dtype, const float* thresholds, int32_t N, int32_t C,
                                  int32_t channel, int64_t HW, int32_t pr_num, uint32_t* hist, void* stream) {
  if (!src || !gt || !thresholds || !hist || N <= 0 || HW <= 0 || pr_num <= 0 || C < 0 || C == 1) return CAVP_ERR_BAD_ARG;
  if (C >= 2 && (channel < 0 || channel >= C)) return CAVP_ERR_BAD_ARG;
  if (src_image_stride < (C >= 2 ? (int64_t)C * HW : HW) && N > 1) return CAVP_ERR_BAD_ARG;
  if (pr_num > CAVP_FMEASURE_MAX_THRESHOLDS) return CAVP_ERR_UNSUPPORTED;
  if (!label_ok(gt_dtype)) return CAVP_ERR_UNSUPPORTED;
  if (((uintptr_t)src & 3) || !label_aligned(gt, gt_dtype) || ((uintptr_t)thresholds & 3) || ((uintptr_t)hist & 3)) return CAVP_ERR_ALIGN;
  const dim3 grid(chunks_for(HW, 4 * kThreads, 256), N);
  const size_t shm = (size_t)(pr_num + 2 * (pr_num + 1)) * sizeof(unsigned);
  hipStream_t s = (hipStream_t)stream;
  dispatch_label(gt_dtype, [&](auto g) { using TG = decltype(g);
    fmeasure_hist_kernel<TG><<<grid, kThreads, shm, s>>>(src, src_image_stride, (const TG*)gt, thresholds, C, channel, HW, pr_num, hist); });
  CHECK_LAUNCH();
}

extern "C" int cavp_clipval_frame_counts(const void* pred, int32_t pred_is_mask, const int64_t* labels, const void* count,
                                         int32_t count_i64, int32_t B, int32_t T, int32_t C, int64_t HW, int32_t K, int64_t ignore,
                                         uint32_t* hist, uint32_t* conf, int64_t* state, void* stream) {
  if (!pred || !labels || !hist || !conf || !state || B <= 0 || T <= 0 || HW <= 0 || K <= 0 || (!pred_is_mask && C <= 0))
    return CAVP_ERR_BAD_ARG;
  if (ignore < 0 || ignore >= kLabelBins) return CAVP_ERR_BAD_ARG;
  if ((long long)B * T > 65535 || HW > 0x7fffffffLL) return CAVP_ERR_UNSUPPORTED;   // grid.y; u32 counts per frame
  if (!classes_ok(K, pred_is_mask ? 0 : C)) return CAVP_ERR_UNSUPPORTED;            // a mask has no channels
  if (((uintptr_t)labels & 7) || ((uintptr_t)hist & 3) || ((uintptr_t)conf & 3) || ((uintptr_t)state & 7) ||
      (!pred_is_mask && ((uintptr_t)pred & 3)) || !aligned_for(count, count_i64 != 0))
    return CAVP_ERR_ALIGN;
  const bool vec = (HW & 3) == 0 && al16(labels) && (pred_is_mask ? ((uintptr_t)pred & 3) == 0 : al16(pred));
  const bool lds = counts_fit_lds(K);
  // 2 quads per thread (25 workgroups per frame at 224^2): enough workgroups for a single clip, few enough LDS clears and flushes
  const dim3 grid(chunks_for((HW + 3) >> 2, 2 * kThreads, 64), B * T);
  const size_t shm = (size_t)(kLabelBins + (lds ? (K + 1) * K : 0)) * sizeof(unsigned);
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_bool(pred_is_mask != 0, [&](auto m) { cavp_dispatch_bool(vec, [&](auto v) { cavp_dispatch_bool(lds, [&](auto l) {
    constexpr bool kMask = decltype(m)::value, kVec = decltype(v)::value, kLds = decltype(l)::value;
    clipval_frame_allow_lds<kMask, kVec, kLds>();
    clipval_frame_kernel<kMask, kVec, kLds><<<grid, kThreads, shm, s>>>(pred, (const long long*)labels, count, count_i64, T, C, HW, K,
                                                                        (int)ignore, hist, conf, (unsigned long long*)state); }); }); });
  CHECK_LAUNCH();
}

extern "C" int cavp_clipval_combine(uint32_t* hist, uint32_t* conf, uint32_t* flags, const void* count, int32_t count_i64, int32_t B,
                                    int32_t T, int32_t K, int32_t min_count, int32_t min_values, uint64_t* counts, int64_t* frames,
                                    int64_t* state, void* stream) {
  if (!hist || !conf || !flags || !counts || !frames || !state || B <= 0 || T <= 0 || K <= 0 || min_count < 0 || min_values < 0)
    return CAVP_ERR_BAD_ARG;
  if ((long long)B * T > 65535 || !classes_ok(K, 0)) return CAVP_ERR_UNSUPPORTED;
  if (((uintptr_t)hist & 3) || ((uintptr_t)conf & 3) || ((uintptr_t)flags & 3) || ((uintptr_t)counts & 7) || ((uintptr_t)frames & 7) ||
      ((uintptr_t)state & 7) || !aligned_for(count, count_i64 != 0))
    return CAVP_ERR_ALIGN;
  const int N = B * T, nbins = (K + 1) * K;
  hipStream_t s = (hipStream_t)stream;
  clipval_flags_kernel<<<N, kLabelBins, 0, s>>>(hist, flags, count, count_i64, T, (unsigned)min_count, min_values,
                                               (unsigned long long*)frames, (unsigned long long*)state);
  const dim3 grid((nbins + kThreads - 1) / kThreads, (N + kCombineFrames - 1) / kCombineFrames);
  clipval_combine_kernel<<<grid, kThreads, 0, s>>>(conf, flags, N, nbins, (unsigned long long*)counts);
  CHECK_LAUNCH();
}

// LDS words of a videoval frame workgroup: thresholds, both histograms and (lds) the confusion counts
static size_t videoval_frame_words(int pr_num, int K, bool lds) { return (size_t)pr_num + 2 * ((size_t)pr_num + 1) + (lds ? (size_t)(K + 1) * K : 0); }

extern "C" int cavp_videoval_frame_stats(const void* pred, int32_t pred_is_mask, const float* prob, const int64_t* labels, const void* count,
                                         int32_t count_i64, int32_t B, int32_t T, int32_t C, int32_t channel, int64_t HW, int32_t K,
                                         int64_t ignore, const float* thresholds, int32_t pr_num, int64_t* stats, uint32_t* hist,
                                         uint64_t* M, int64_t* state, void* stream) {
  if (!pred || !labels || !thresholds || !stats || !hist || !M || !state || B <= 0 || T <= 0 || HW <= 0 || K <= 0 || pr_num <= 0)
    return CAVP_ERR_BAD_ARG;
  if (pred_is_mask ? !prob : (C < 2 || channel < 0 || channel >= C)) return CAVP_ERR_BAD_ARG;
  if ((long long)B * T > 65535 || HW > 0x7fffffffLL || pr_num > CAVP_VIDEOVAL_MAX_THRESHOLDS) return CAVP_ERR_UNSUPPORTED;   // grid.y; u32 counts
  if (!classes_ok(K, pred_is_mask ? 0 : C)) return CAVP_ERR_UNSUPPORTED;   // a mask has no channels
  if (((uintptr_t)labels & 7) || ((uintptr_t)stats & 7) || ((uintptr_t)hist & 3) || ((uintptr_t)M & 7) || ((uintptr_t)state & 7) ||
      ((uintptr_t)thresholds & 3) || (pred_is_mask ? ((uintptr_t)prob & 3) != 0 : ((uintptr_t)pred & 3) != 0) ||
      !aligned_for(count, count_i64 != 0))
    return CAVP_ERR_ALIGN;
  const bool vec = (HW & 3) == 0 && al16(labels) && (pred_is_mask ? ((uintptr_t)pred & 3) == 0 && al16(prob) : al16(pred));
  // the confusion counts are privatised when they fit the default 64 KiB beside the thresholds and the histograms (K <= 124 at 255)
  const bool lds = counts_fit_lds(K) && videoval_frame_words(pr_num, K, true) <= (size_t)kLdsBins;
  // 2 quads per thread, as clipval_frame_kernel: 25 workgroups per frame at 224^2
  const dim3 grid(chunks_for((HW + 3) >> 2, 2 * kThreads, 64), B * T);
  const size_t shm = videoval_frame_words(pr_num, K, lds) * sizeof(unsigned);
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_bool(pred_is_mask != 0, [&](auto m) { cavp_dispatch_bool(vec, [&](auto v) { cavp_dispatch_bool(lds, [&](auto l) {
    videoval_frame_kernel<decltype(m)::value, decltype(v)::value, decltype(l)::value><<<grid, kThreads, shm, s>>>(
        pred, prob, (const long long*)labels, count, count_i64, T, C, channel, HW, K, ignore, thresholds, pr_num,
        (unsigned long long*)stats, hist, (unsigned long long*)M, (unsigned long long*)state); }); }); });
  CHECK_LAUNCH();
}

extern "C" int cavp_videoval_combine(int64_t* stats, uint32_t* hist, const void* count, int32_t count_i64, int32_t B, int32_t T, int64_t HW,
                                     int32_t pr_num, int32_t max_videos, float* J, float* F, int64_t* state, void* stream) {
  if (!stats || !hist || !J || !F || !state || B <= 0 || T <= 0 || HW <= 0 || pr_num <= 0 || max_videos <= 0) return CAVP_ERR_BAD_ARG;
  if ((long long)B * T > 65535 || HW > 0x7fffffffLL || pr_num > CAVP_VIDEOVAL_MAX_THRESHOLDS) return CAVP_ERR_UNSUPPORTED;
  if (((uintptr_t)stats & 7) || ((uintptr_t)hist & 3) || ((uintptr_t)J & 3) || ((uintptr_t)F & 3) || ((uintptr_t)state & 7) ||
      !aligned_for(count, count_i64 != 0))
    return CAVP_ERR_ALIGN;
  const size_t shm = videoval_combine_words(pr_num) * sizeof(unsigned);
  videoval_combine_kernel<<<B, kThreads, shm, (hipStream_t)stream>>>((unsigned long long*)stats, hist, count, count_i64, B, T, HW, pr_num,
                                                                      max_videos, J, F, (unsigned long long*)state);
  CHECK_LAUNCH();
}

static bool semval_shape_ok(int B, int T, int64_t HW, int K) {
  return (long long)B * T <= 65535 && HW <= 0x7fffffffLL && K >= 2 && K <= CAVP_METRICS_MAX_CLASSES;   // grid.y; u32 counts; histc
}

extern "C" int cavp_semval_frame_counts(const void* pred, int32_t pred_is_mask, const int64_t* labels, const void* count,
                                        int32_t count_i64, int32_t B, int32_t T, int32_t C, int64_t HW, int32_t K, uint32_t* scratch,
                                        int64_t* state, void* stream) {
  if (!pred || !labels || !scratch || !state || B <= 0 || T <= 0 || HW <= 0 || K <= 0) return CAVP_ERR_BAD_ARG;
  if (!pred_is_mask && C != K) return CAVP_ERR_BAD_ARG;   // the metric takes its class number from the logits
  if (!semval_shape_ok(B, T, HW, K)) return CAVP_ERR_UNSUPPORTED;
  if (((uintptr_t)labels & 7) || ((uintptr_t)scratch & 3) || ((uintptr_t)state & 7) || (!pred_is_mask && ((uintptr_t)pred & 3)) ||
      !aligned_for(count, count_i64 != 0))
    return CAVP_ERR_ALIGN;
  const bool vec = (HW & 3) == 0 && al16(labels) && (pred_is_mask ? ((uintptr_t)pred & 3) == 0 : al16(pred));
  // 2 quads per thread, as clipval_frame_kernel: 25 workgroups per frame at 224^2, each clears and flushes 3K + 4 counters
  const dim3 grid(chunks_for((HW + 3) >> 2, kSemvalQuads * kThreads, 1 << 20), B * T);
  const size_t shm = (size_t)(3 * K + 4) * sizeof(unsigned);   // at most 48 KiB + 16 bytes: always in LDS
  hipStream_t s = (hipStream_t)stream;
  cavp_dispatch_bool(pred_is_mask != 0, [&](auto m) { cavp_dispatch_bool(vec, [&](auto v) {
    semval_frame_kernel<decltype(m)::value, decltype(v)::value><<<grid, kThreads, shm, s>>>(
        pred, (const long long*)labels, count, count_i64, T, HW, K, scratch, (unsigned long long*)state); }); });
  CHECK_LAUNCH();
}

extern "C" int cavp_semval_combine(uint32_t* scratch, const void* count, int32_t count_i64, int32_t B, int32_t T, int64_t HW, int32_t K,
                                   int32_t max_frames, float* acc, float* last, int64_t* state, void* stream) {
  if (!scratch || !acc || !last || !state || B <= 0 || T <= 0 || HW <= 0 || K <= 0 || max_frames <= 0) return CAVP_ERR_BAD_ARG;
  if ((long long)B * T > max_frames) return CAVP_ERR_BAD_ARG;
  if (!semval_shape_ok(B, T, HW, K)) return CAVP_ERR_UNSUPPORTED;
  if (((uintptr_t)scratch & 3) || ((uintptr_t)acc & 3) || ((uintptr_t)last & 3) || ((uintptr_t)state & 7) ||
      !aligned_for(count, count_i64 != 0))
    return CAVP_ERR_ALIGN;
  semval_combine_kernel<<<(K + kSemvalCombineThreads - 1) / kSemvalCombineThreads, kSemvalCombineThreads, 0, (hipStream_t)stream>>>(
      scratch, count, count_i64, B, T, HW, K, max_frames, acc, last, (unsigned long long*)state);
  CHECK_LAUNCH();
}
