// Device side of the pixel-level audio-visual InfoNCE (reference loss/contrastive_aud.py::ContrastLoss.info_nce and
// the normalise / gather part of ::forward / ::extraction_samples).  By default the class-balanced SAMPLING stays on the host
// (it consumes torch.randperm from the CPU generator; reproducing the reference's indices needs the same RNG stream);
// the host hands over (image, pixel) index lists + labels of the N <= ~3000 anchors.  The opt-in device sampler (second half
// of this file) picks the anchors here, with Philox keys.  Every kernel of the chain takes its anchor count from anchor_count():
// the sampler's plan header on the device, or the host's (N, n_match) when there is no header.
//   1. gather_l2norm:   A[i] = x[b_i, :, p_i] / max(||.||_2, eps)         (F.normalize(dim=1) then boolean gather)
//   2. S = A A^T / T:   the f32 MFMA igemm (cavp_conv2d_nhwc, weights = A)
//   3. infonce_rows:    one workgroup per anchor row: max, negative sum, per-positive log-prob, mean; optional dS
//   4. symm_add:        G = dS + dS^T  (anchors and contrasts are the same tensor: both roles get gradient)
//   5. dA = G A (cavp_conv2d_wgrad_nhwc), then l2norm_bwd_scatter back into the NHWC feature gradient
#include "common.h"
#include "host_util.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The anchor count of a launch: from the device sampler's plan header (cap = the plan's capacity; N / n_match ignored) or,
// header == nullptr, from the host.  Rows < n_match belong to the match half, the others to the shuffle half.
struct AnchorCount { int n, n_match; };
__device__ __forceinline__ AnchorCount anchor_count(const int* __restrict__ header, int cap, int N, int n_match) {
  if (!header) return {N, n_match};
  int n = header[0];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  return {n, header[1]};
}

// one wave per row of A; rows >= n are zero (norm 1)
__global__ __launch_bounds__(256) void gather_l2norm_kernel(const float* __restrict__ xm, long long msb, long long msc, long long msp,
                                                            const float* __restrict__ xs, long long ssb, long long ssc, long long ssp,
                                                            const int* __restrict__ header, const int* __restrict__ ib,
                                                            const int* __restrict__ ip, int cap, int N, int n_match, int rows, int C,
                                                            float eps, float* __restrict__ A, float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const AnchorCount cnt = anchor_count(header, cap, N, n_match);
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += gridDim.x * 4) {
    if (i >= cnt.n) {
      for (int c = lane; c < C; c += 64) A[(size_t)i * C + c] = 0.f;
      if (lane == 0) norms[i] = 1.f;
      continue;
    }
    const bool m = i < cnt.n_match;
    const long long sc = m ? msc : ssc;
    const float* src = m ? xm + (long long)ib[i] * msb + (long long)ip[i] * msp : xs + (long long)ib[i] * ssb + (long long)ip[i] * ssp;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float v = src[(long long)c * sc]; q += v * v; }
    const float nrm = fmaxf(sqrtf(wave_sum(q)), eps);
    for (int c = lane; c < C; c += 64) A[(size_t)i * C + c] = src[(long long)c * sc] / nrm;
    if (lane == 0) norms[i] = nrm;
  }
}

// S: [ld][ld] (row i = anchor i, already divided by the temperature); labels: int [N]
// out_rows[i] = mean_log_prob_pos_i; dS (optional) = d(-mean_i mlpp_i)/dS * grad_scale, zero outside [N][N]
__device__ __forceinline__ void infonce_row(const float* __restrict__ S, const int* __restrict__ lab, int N, int ld, float eps,
                                            float* __restrict__ out_rows, float* __restrict__ dS, float grad_scale, float* red) {
  const int i = blockIdx.x;
  if (i >= ld) return;
  if (i >= N) {  // padding row
    if (dS) for (int j = threadIdx.x; j < ld; j += 256) dS[(size_t)i * ld + j] = 0.f;
    return;
  }
  const float* row = S + (size_t)i * ld;
  const int li = lab[i];
  float m = -INFINITY;
  for (int j = threadIdx.x; j < N; j += 256) m = fmaxf(m, row[j]);
  m = block_max(m, red);
  float neg = 0.f, cnt = 0.f;
  for (int j = threadIdx.x; j < N; j += 256) {
    const bool same = lab[j] == li;
    neg += same ? 0.f : expf(row[j] - m);
    cnt += (same && j != i) ? 1.f : 0.f;
  }
  neg = block_sum(neg, red);
  cnt = block_sum(cnt, red);
  float slp = 0.f, rsum = 0.f;
  for (int j = threadIdx.x; j < N; j += 256) {
    if (lab[j] == li && j != i) {
      const float l = row[j] - m, e = expf(l);
      slp += l - logf(e + neg);
      rsum += 1.f / (e + neg);
    }
  }
  slp = block_sum(slp, red);
  rsum = block_sum(rsum, red);
  if (threadIdx.x == 0) out_rows[i] = slp / (cnt + eps);
  if (dS) {
    // d(-1/N sum_i mlpp_i)/dl_ik = -c_i [ m_ik (1 - e_ik / D_ik) - e_ik n_ik R_i ],  c_i = 1 / (N (P_i + eps))
    const float ci = grad_scale / ((float)N * (cnt + eps));
    for (int j = threadIdx.x; j < ld; j += 256) {
      float g = 0.f;
      if (j < N) {
        const float e = expf(row[j] - m);
        const bool same = lab[j] == li;
        if (same && j != i) g = -ci * (1.f - e / (e + neg));
        if (!same) g = ci * e * rsum;
      }
      dS[(size_t)i * ld + j] = g;
    }
  }
}

__global__ __launch_bounds__(256) void infonce_rows_kernel(const float* __restrict__ S, const int* __restrict__ lab,
                                                           const int* __restrict__ header, int cap, int N, int ld, float eps,
                                                           float* __restrict__ out_rows, float* __restrict__ dS, float grad_scale) {
  __shared__ float red[4];
  infonce_row(S, lab, anchor_count(header, cap, N, 0).n, ld, eps, out_rows, dS, grad_scale, red);
}

// loss = -mean(rows[0 .. n)); 0 when the plan is empty
__global__ __launch_bounds__(256) void mean_neg_kernel(const float* rows, const int* __restrict__ header, int cap, int N, float* loss) {
  __shared__ float red[4];
  const int n = anchor_count(header, cap, N, 0).n;
  float s = 0.f;
  for (int j = threadIdx.x; j < n; j += 256) s += rows[j];
  s = block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = n > 0 ? -s / (float)n : 0.f;
}

__global__ __launch_bounds__(256) void symm_add_kernel(const float* __restrict__ d, float* __restrict__ g, int n,
                                                       float scale, const float* __restrict__ scale_dev) {
  if (scale_dev) scale *= *scale_dev;   // the upstream gradient of the loss, read on the device (no host round trip)
  const long long total = (long long)n * n;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int i = (int)(t / n), j = (int)(t - (long long)i * n);
    g[t] = (d[t] + d[(size_t)j * n + i]) * scale;
  }
}

// dx[b_i, :, p_i] = (dA_i - A_i <A_i, dA_i>) / ||x_i||   (anchors are distinct pixels per half: plain scatter)
__global__ __launch_bounds__(256) void l2norm_bwd_scatter_kernel(const float* __restrict__ dA, const float* __restrict__ A,
                                                                 const float* __restrict__ norms, const int* __restrict__ header,
                                                                 const int* __restrict__ ib, const int* __restrict__ ip, int cap, int N,
                                                                 int n_match, int C,
                                                                 float* __restrict__ dxm, long long msb, long long msc, long long msp,
                                                                 float* __restrict__ dxs, long long ssb, long long ssc, long long ssp) {
  const int lane = threadIdx.x & 63;
  const AnchorCount cnt = anchor_count(header, cap, N, n_match);
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt.n; i += gridDim.x * 4) {
    float dot = 0.f;
    for (int c = lane; c < C; c += 64) dot += A[(size_t)i * C + c] * dA[(size_t)i * C + c];
    dot = wave_sum(dot);
    const float inv = 1.f / norms[i];
    const bool m = i < cnt.n_match;
    const long long sc = m ? msc : ssc;
    float* dst = m ? dxm + (long long)ib[i] * msb + (long long)ip[i] * msp : dxs + (long long)ib[i] * ssb + (long long)ip[i] * ssp;
    for (int c = lane; c < C; c += 64) dst[(long long)c * sc] = (dA[(size_t)i * C + c] - A[(size_t)i * C + c] * dot) * inv;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Device-side anchor sampling (include/cavp_hip.h, ABI 14).  count -> plan -> select, then the chain above with the anchor
// count read from the plan header.  Nothing here depends on the order in which atomics arrive: the histograms are integer
// counts, and the candidates that the LDS slot counter hands out in arrival order are sorted by their unique (key, i).
constexpr int kHistStride = 257;      // 256 label bins + one for labels outside [0, 255]
constexpr int kCountBlocks = 64;      // per-workgroup partial histograms, added in workgroup order by the plan kernel
constexpr int kSelThreads = 1024;
constexpr int kSelBits = 12;          // radix digit of the threshold search
constexpr int kSelList = 2048;        // candidates sorted in LDS: < max_views <= 1024 below the boundary digit + <= 1024 inside it

// (philox_key: common.h, shared with pairs.hip)

__global__ __launch_bounds__(256) void contrast_count_kernel(const int* __restrict__ gm, long long total, int* __restrict__ partial) {
  __shared__ unsigned hist[kHistStride];
  for (int c = threadIdx.x; c < kHistStride; c += 256) hist[c] = 0u;
  __syncthreads();
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int l = gm[i];
    atomicAdd(&hist[(l >= 0 && l <= 255) ? l : 256], 1u);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < kHistStride; c += 256) partial[blockIdx.x * kHistStride + c] = (int)hist[c];
}

// groups (each int32[G], G = max_classes + 2): label (class, 0 = background, -1 = all foreground), q, first row
__global__ __launch_bounds__(256) void contrast_plan_kernel(const int* __restrict__ partial, int nparts, int ignore_idx, int max_views,
                                                            int max_classes, long long* __restrict__ state, int* __restrict__ header,
                                                            int* __restrict__ gl, int* __restrict__ gq, int* __restrict__ grow) {
  __shared__ int cnt[kHistStride];
  for (int c = threadIdx.x; c < kHistStride; c += 256) {
    int s = 0;
    for (int b = 0; b < nparts; ++b) s += partial[b * kHistStride + c];
    cnt[c] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int G = max_classes + 2;
  int kept = 0, qualify = 0, row = 0;
  long long n_fg = 0;
  for (int c = 1; c < 256; ++c) {
    if (c == ignore_idx) continue;
    n_fg += cnt[c];
    if (cnt[c] >= max_views) {
      ++qualify;
      if (kept < max_classes) { gl[kept] = c; gq[kept] = max_views; grow[kept] = row; row += max_views; ++kept; }
    }
  }
  int sample_num = 0, used = 0;
  if (kept > 0) {
    const long long m = n_fg < (long long)cnt[0] ? n_fg : (long long)cnt[0];
    sample_num = m < (long long)max_views ? (int)m : max_views;
    gl[kept] = 0; gq[kept] = sample_num; grow[kept] = row; row += sample_num;
    gl[kept + 1] = -1; gq[kept + 1] = sample_num; grow[kept + 1] = row; row += sample_num;
    used = kept + 2;
  }
  for (int g = used; g < G; ++g) { gl[g] = 0; gq[g] = 0; grow[g] = 0; }
  const long long seed = state[0], off = state[1];
  header[0] = row;
  header[1] = row - sample_num;
  header[2] = kept;
  header[3] = sample_num;
  header[4] = (int)(unsigned)((unsigned long long)off & 0xffffffffull);
  header[5] = (int)(unsigned)((unsigned long long)off >> 32);
  header[6] = (int)(unsigned)((unsigned long long)seed & 0xffffffffull);
  header[7] = (int)(unsigned)((unsigned long long)seed >> 32);
  state[1] = off + 1;
  state[2] += qualify > max_classes ? qualify - max_classes : 0;
  state[3] += cnt[256];
}

__device__ __forceinline__ bool sel_member(int l, int kind, int ignore_idx) {
  return kind >= 0 ? l == kind : (l > 0 && l <= 255 && l != ignore_idx);
}

// One workgroup per group.  Threshold search: histogram one radix digit of the members' keys, take the digit in which the q-th
// smallest key lies, descend into it while it still holds more than 1024 members (for uniform keys: only when a group has
// millions of pixels).  Then every member at or below the threshold prefix goes into LDS (< q below the boundary digit, <= 1024
// inside it), is sorted by (key, i), and the first q are the pick.  The label map is streamed once per pass; keys are recomputed.
__global__ __launch_bounds__(kSelThreads) void contrast_select_kernel(const int* __restrict__ gm, const int* __restrict__ gs, long long total,
                                                                      int HW, int ignore_idx, const int* __restrict__ header,
                                                                      const int* __restrict__ gl, const int* __restrict__ gq,
                                                                      const int* __restrict__ grow, int cap, int* __restrict__ idx_b,
                                                                      int* __restrict__ idx_p, int* __restrict__ labels) {
  __shared__ unsigned hist[1 << kSelBits];
  __shared__ unsigned long long skey[kSelList];
  __shared__ int sidx[kSelList];
  __shared__ unsigned wtot[kSelThreads / 64];
  __shared__ unsigned s_bin, s_below, s_cnt, s_n;
  const int g = blockIdx.x, tid = threadIdx.x;
  int n = header[0];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  for (long long r = (long long)n + (long long)g * kSelThreads + tid; r < cap; r += (long long)gridDim.x * kSelThreads) {
    idx_b[r] = -1; idx_p[r] = -1; labels[r] = -1;
  }
  const int q = gq[g] < kSelThreads ? gq[g] : kSelThreads;
  if (q <= 0) return;
  const int kind = gl[g], row0 = grow[g];
  const unsigned stream = kind > 0 ? 0u : (kind == 0 ? 1u : 2u);
  const unsigned off_lo = (unsigned)header[4], off_hi = (unsigned)header[5], k0 = (unsigned)header[6], k1 = (unsigned)header[7];

  unsigned long long prefix = 0;
  int pbits = 0;
  unsigned need = (unsigned)q;
  for (;;) {
    const int w = 64 - pbits < kSelBits ? 64 - pbits : kSelBits, shift = 64 - pbits - w;
    for (int b = tid; b < (1 << kSelBits); b += kSelThreads) hist[b] = 0u;
    if (tid == 0) { s_bin = (1u << w) - 1u; s_below = 0u; s_cnt = 0u; }
    __syncthreads();
    for (long long i = tid; i < total; i += kSelThreads) {
      if (!sel_member(gm[i], kind, ignore_idx)) continue;
      const unsigned long long key = philox_key((unsigned)i, stream, off_lo, off_hi, k0, k1);
      if (pbits == 0 || (key >> (64 - pbits)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & ((1u << w) - 1u)], 1u);
    }
    __syncthreads();
    // the digit b with cum(b - 1) < need <= cum(b): every thread owns 4 consecutive bins
    unsigned h4[4], t = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h4[e] = hist[tid * 4 + e]; t += h4[e]; }
    unsigned inc = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(inc, o, 64);
      if ((tid & 63) >= o) inc += v;
    }
    if ((tid & 63) == 63) wtot[tid >> 6] = inc;
    __syncthreads();
    unsigned ex = inc - t;
    for (int v = 0; v < (tid >> 6); ++v) ex += wtot[v];
    if (ex < need && need <= ex + t) {
      unsigned c = ex;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c < need && need <= c + h4[e]) { s_bin = (unsigned)(tid * 4 + e); s_below = c; s_cnt = h4[e]; }
        c += h4[e];
      }
    }
    __syncthreads();
    const unsigned bin = s_bin, below = s_below, cntb = s_cnt;
    prefix = (prefix << w) | bin;
    pbits += w;
    if (cntb <= 1024u || pbits >= 64) break;
    need -= below;
    __syncthreads();
  }

  for (int e = tid; e < kSelList; e += kSelThreads) { skey[e] = ~0ull; sidx[e] = 0x7fffffff; }
  if (tid == 0) s_n = 0u;
  __syncthreads();
  for (long long i = tid; i < total; i += kSelThreads) {
    if (!sel_member(gm[i], kind, ignore_idx)) continue;
    const unsigned long long key = philox_key((unsigned)i, stream, off_lo, off_hi, k0, k1);
    if ((key >> (64 - pbits)) <= prefix) {
      const unsigned slot = atomicAdd(&s_n, 1u);
      if (slot < (unsigned)kSelList) { skey[slot] = key; sidx[slot] = (int)i; }
    }
  }
  __syncthreads();
  // bitonic sort of the kSelList (key, i) pairs, ascending; the padding (key ~0, i INT_MAX) sorts last
  for (int k = 2; k <= kSelList; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int a = 2 * tid - (tid & (j - 1)), b = a + j;
      const unsigned long long ka = skey[a], kb = skey[b];
      const int ia = sidx[a], ib = sidx[b];
      const bool gt = ka > kb || (ka == kb && ia > ib);
      if (gt == ((a & k) == 0)) { skey[a] = kb; skey[b] = ka; sidx[a] = ib; sidx[b] = ia; }
      __syncthreads();
    }
  }
  if (tid < q && row0 + tid < cap) {
    const int i = sidx[tid];
    if (i >= 0 && (long long)i < total) {
      const int r = row0 + tid;
      idx_b[r] = i / HW;
      idx_p[r] = i - (i / HW) * HW;
      labels[r] = kind > 0 ? kind : (kind == 0 ? 0 : gs[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The two ends of the chain on the training tape's fusion map as it lies in memory: x / g = [2B][HW][ld] of the compute dtype
// (ld >= C, the match half first).  Anchor i lives in image idx_b[i] (i < n_match) or B + idx_b[i]; the count comes from the
// device sampler's header or, header == nullptr, from the host.  One wave per anchor row, 16-byte vectors, f32 arithmetic.
// first element of anchor i's row, or -1 when the plan entry does not address a pixel of the map (rows >= n hold -1)
__device__ __forceinline__ long long anchor_row(const int* __restrict__ ib, const int* __restrict__ ip, int i, int n_match, int B,
                                                int HW, int ld) {
  const int b = ib[i], p = ip[i];
  if ((unsigned)b >= (unsigned)B || (unsigned)p >= (unsigned)HW) return -1;
  return ((long long)(b + (i < n_match ? 0 : B)) * HW + p) * ld;
}

template <typename T>
__global__ __launch_bounds__(256) void contrast_gather_nhwc_kernel(const T* __restrict__ x, int B, int HW, int ld, int C,
                                                                   const int* __restrict__ header, const int* __restrict__ ib,
                                                                   const int* __restrict__ ip, int cap, int N, int n_match,
                                                                   int rows, float eps, float* __restrict__ A,
                                                                   float* __restrict__ norms) {
  constexpr int VE = VecT<T>::VE;
  const int lane = threadIdx.x & 63, CV = C / VE;
  const AnchorCount cnt = anchor_count(header, cap, N, n_match);
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += gridDim.x * 4) {
    float* dst = A + (size_t)i * C;
    const long long off = i < cnt.n ? anchor_row(ib, ip, i, cnt.n_match, B, HW, ld) : -1;
    if (off < 0) {
      for (int c = lane * 4; c < C; c += 256) *(float4*)(dst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane == 0) norms[i] = 1.f;
      continue;
    }
    const T* src = x + off;
    float q = 0.f, v[VE];
    for (int cv = lane; cv < CV; cv += 64) {
      VecT<T>::load(src + cv * VE, v);
#pragma unroll
      for (int e = 0; e < VE; ++e) q += v[e] * v[e];
    }
    const float nrm = fmaxf(sqrtf(wave_sum(q)), eps);
    for (int cv = lane; cv < CV; cv += 64) {   // (the row is a few hundred bytes: the second read comes from the cache)
      VecT<T>::load(src + cv * VE, v);
#pragma unroll
      for (int e = 0; e < VE; e += 4)
        *(float4*)(dst + cv * VE + e) = make_float4(v[e] / nrm, v[e + 1] / nrm, v[e + 2] / nrm, v[e + 3] / nrm);
    }
    if (lane == 0) norms[i] = nrm;
  }
}

// g_row += scale * (dA_i - A_i <A_i, dA_i>) / norms[i]; the anchors are distinct pixels per half: plain read-modify-write
template <typename T>
__global__ __launch_bounds__(256) void contrast_rows_bwd_add_kernel(T* __restrict__ g, int B, int HW, int ld, int C,
                                                                    const int* __restrict__ header, const int* __restrict__ ib,
                                                                    const int* __restrict__ ip, int cap, int N, int n_match,
                                                                    const float* __restrict__ dA, const float* __restrict__ A,
                                                                    const float* __restrict__ norms, float scale) {
  constexpr int VE = VecT<T>::VE;
  const int lane = threadIdx.x & 63, CV = C / VE;
  const AnchorCount cnt = anchor_count(header, cap, N, n_match);
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt.n; i += gridDim.x * 4) {
    const long long off = anchor_row(ib, ip, i, cnt.n_match, B, HW, ld);
    if (off < 0) continue;
    const float* a = A + (size_t)i * C;
    const float* d = dA + (size_t)i * C;
    float dot = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
      const float4 av = *(const float4*)(a + c), dv = *(const float4*)(d + c);
      dot += av.x * dv.x + av.y * dv.y + av.z * dv.z + av.w * dv.w;
    }
    dot = wave_sum(dot);
    const float inv = scale / norms[i];
    T* dst = g + off;
    for (int cv = lane; cv < CV; cv += 64) {
      float v[VE];
      VecT<T>::load(dst + cv * VE, v);
#pragma unroll
      for (int e = 0; e < VE; e += 4) {
        const float4 av = *(const float4*)(a + cv * VE + e), dv = *(const float4*)(d + cv * VE + e);
        v[e] += (dv.x - av.x * dot) * inv;
        v[e + 1] += (dv.y - av.y * dot) * inv;
        v[e + 2] += (dv.z - av.z * dot) * inv;
        v[e + 3] += (dv.w - av.w * dot) * inv;
      }
      VecT<T>::store(dst + cv * VE, v);
    }
  }
}

}  // namespace

// F.interpolate(mode='nearest') of the label maps to the feature resolution (contrastive_aud.py:18-22): source index
// min(floor(dst * float32(in / out)), in - 1) per axis, as ATen computes it.  int64 [B][H][W] -> int32 [B][h][w].
static __global__ __launch_bounds__(256) void label_nearest_kernel(const long long* __restrict__ gt, int* __restrict__ out, int B,
                                                                   int H, int W, int h, int w, float sh, float sw) {
  const long long total = (long long)B * h * w;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % w), y = (int)((i / w) % h), b = (int)(i / ((long long)w * h));
    int ys = (int)floorf((float)y * sh), xs = (int)floorf((float)x * sw);
    ys = ys < H - 1 ? ys : H - 1;
    xs = xs < W - 1 ? xs : W - 1;
    out[i] = (int)gt[((size_t)b * H + ys) * W + xs];
  }
}

extern "C" int cavp_label_nearest(const int64_t* gt, int32_t* out, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w,
                                  void* stream) {
  if (!gt || !out || B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return CAVP_ERR_BAD_ARG;
  const long long total = (long long)B * h * w;
  long long nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  label_nearest_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>((const long long*)gt, out, B, H, W, h, w, (float)H / (float)h,
                                                                 (float)W / (float)w);
  CHECK_LAUNCH();
}

// shared argument check of the chain's strided-f32 ends: the count from `header` (cap rows of plan) or from (N, n_match).
// map_m / map_s: the two feature maps (gather) or their gradients (scatter); rows0 / rows1: the [rows][C] buffers of the call
// (gather: A twice; scatter: dA and A)
static int contrast_ends_args_ok(const float* map_m, const float* map_s, const int32_t* header, const int32_t* idx_b,
                                 const int32_t* idx_p, int cap, int N, int n_match, int C, const float* rows0, const float* rows1,
                                 const float* norms) {
  if (!map_m || !map_s || !idx_b || !idx_p || !rows0 || !rows1 || !norms || C <= 0) return CAVP_ERR_BAD_ARG;
  if (header ? cap <= 0 : (N <= 0 || n_match < 0 || n_match > N)) return CAVP_ERR_BAD_ARG;
  return CAVP_OK;
}

extern "C" int cavp_gather_l2norm(const float* xm, int64_t m_stride_b, int64_t m_stride_c, int64_t m_stride_p, const float* xs,
                                  int64_t s_stride_b, int64_t s_stride_c, int64_t s_stride_p, const int32_t* header,
                                  const int32_t* idx_b, const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match, int32_t rows,
                                  int32_t C, float eps, float* A, float* norms, void* stream) {
  const int st = contrast_ends_args_ok(xm, xs, header, idx_b, idx_p, cap, N, n_match, C, A, A, norms);
  if (st != CAVP_OK) return st;
  if (rows < (header ? cap : N)) return CAVP_ERR_BAD_ARG;
  gather_l2norm_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(xm, m_stride_b, m_stride_c, m_stride_p, xs, s_stride_b, s_stride_c,
                                                                        s_stride_p, header, idx_b, idx_p, cap, N, n_match, rows, C, eps,
                                                                        A, norms);
  CHECK_LAUNCH();
}

extern "C" int cavp_infonce_rows(const float* S, const int32_t* labels, const int32_t* header, int32_t cap, int32_t N, int32_t ld,
                                 float eps, float* row_mlpp, float* loss, float* dS, float grad_scale, void* stream) {
  if (!S || !labels || !row_mlpp || !loss || (header ? cap <= 0 : N <= 0) || ld < (header ? cap : N)) return CAVP_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  infonce_rows_kernel<<<ld, 256, 0, s>>>(S, labels, header, cap, N, ld, eps, row_mlpp, dS, grad_scale);
  mean_neg_kernel<<<1, 256, 0, s>>>(row_mlpp, header, cap, N, loss);
  CHECK_LAUNCH();
}

extern "C" int cavp_symm_add(const float* d, float* g, int32_t n, float scale, const float* scale_dev, void* stream) {
  if (!d || !g || n <= 0) return CAVP_ERR_BAD_ARG;
  long long nb = ((long long)n * n + 255) / 256;
  if (nb > 8192) nb = 8192;
  symm_add_kernel<<<(int)nb, 256, 0, (hipStream_t)stream>>>(d, g, n, scale, scale_dev);
  CHECK_LAUNCH();
}

extern "C" int cavp_l2norm_bwd_scatter(const float* dA, const float* A, const float* norms, const int32_t* header, const int32_t* idx_b,
                                       const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match, int32_t C, float* dxm,
                                       int64_t m_stride_b, int64_t m_stride_c, int64_t m_stride_p, float* dxs, int64_t s_stride_b,
                                       int64_t s_stride_c, int64_t s_stride_p, void* stream) {
  const int st = contrast_ends_args_ok(dxm, dxs, header, idx_b, idx_p, cap, N, n_match, C, dA, A, norms);
  if (st != CAVP_OK) return st;
  const int rows = header ? cap : N;
  l2norm_bwd_scatter_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(dA, A, norms, header, idx_b, idx_p, cap, N, n_match, C, dxm,
                                                                             m_stride_b, m_stride_c, m_stride_p, dxs, s_stride_b,
                                                                             s_stride_c, s_stride_p);
  CHECK_LAUNCH();
}

// ---- ABI 14: device-side sampling ----
extern "C" size_t cavp_contrast_sample_work_bytes(int32_t max_classes) {
  if (max_classes < 1 || max_classes > 254) return 0;
  return ((size_t)kCountBlocks * kHistStride + 3 * (size_t)(max_classes + 2)) * sizeof(int32_t);
}

extern "C" int cavp_contrast_sample(const int32_t* gm, const int32_t* gs, int64_t total, int32_t HW, int32_t ignore_idx,
                                    int32_t max_views, int32_t max_classes, int64_t* state, int32_t* header, int32_t* work,
                                    int32_t* idx_b, int32_t* idx_p, int32_t* labels, void* stream) {
  if (!gm || !gs || !state || !header || !work || !idx_b || !idx_p || !labels || HW <= 0 || total <= 0) return CAVP_ERR_BAD_ARG;
  if (total > 0x7fffffffll || total % HW != 0 || max_views < 1 || max_views > kSelThreads || max_classes < 1 || max_classes > 254)
    return CAVP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int G = max_classes + 2, cap = G * max_views;
  long long nb = (total + 2047) / 2048;
  if (nb > kCountBlocks) nb = kCountBlocks;
  int* gl = work + kCountBlocks * kHistStride;
  contrast_count_kernel<<<(int)nb, 256, 0, s>>>(gm, total, work);
  contrast_plan_kernel<<<1, 256, 0, s>>>(work, (int)nb, ignore_idx, max_views, max_classes, (long long*)state, header, gl, gl + G,
                                         gl + 2 * G);
  contrast_select_kernel<<<G, kSelThreads, 0, s>>>(gm, gs, total, HW, ignore_idx, header, gl, gl + G, gl + 2 * G, cap, idx_b, idx_p,
                                                   labels);
  CHECK_LAUNCH();
}

// ---- the chain's two ends on the [2B][HW][ld] compute-dtype fusion map of the training tape ----
// shared argument check: C a multiple of 8 (one 16-byte bf16 vector; f32 rows of A / dA then split into float4 as well), ld a
// multiple of the dtype's vector, 16-byte aligned bases; the count from `header` (cap rows of plan) or from (N, n_match)
static int contrast_nhwc_args_ok(int dtype, const void* x, int B, int HW, int ld, int C, const int32_t* header, const int32_t* idx_b,
                                 const int32_t* idx_p, int cap, int N, int n_match, const float* a0, const float* a1,
                                 const float* norms) {
  if (!dt_ok(dtype) || !x || !idx_b || !idx_p || !a0 || !a1 || !norms || B <= 0 || HW <= 0 || C <= 0 || ld < C) return CAVP_ERR_BAD_ARG;
  if (header ? cap <= 0 : (N <= 0 || n_match < 0 || n_match > N)) return CAVP_ERR_BAD_ARG;
  if (C % 8 != 0 || ld % dt_ve(dtype) != 0) return CAVP_ERR_BAD_ARG;
  if (!al16(x) || !al16(a0) || !al16(a1)) return CAVP_ERR_ALIGN;
  return CAVP_OK;
}

extern "C" int cavp_contrast_gather_nhwc(int32_t dtype, const void* x, int32_t B, int32_t HW, int32_t ld, int32_t C,
                                         const int32_t* header, const int32_t* idx_b, const int32_t* idx_p, int32_t cap, int32_t N,
                                         int32_t n_match, int32_t rows, float eps, float* A, float* norms, void* stream) {
  const int st = contrast_nhwc_args_ok(dtype, x, B, HW, ld, C, header, idx_b, idx_p, cap, N, n_match, A, A, norms);
  if (st != CAVP_OK) return st;
  if (rows < (header ? cap : N)) return CAVP_ERR_BAD_ARG;
  cavp_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    contrast_gather_nhwc_kernel<T><<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>((const T*)x, B, HW, ld, C, header, idx_b, idx_p, cap, N,
                                                                                   n_match, rows, eps, A, norms);
  });
  CHECK_LAUNCH();
}

extern "C" int cavp_contrast_rows_bwd_add(int32_t dtype, void* g, int32_t B, int32_t HW, int32_t ld, int32_t C, const int32_t* header,
                                          const int32_t* idx_b, const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match,
                                          const float* dA, const float* A, const float* norms, float scale, void* stream) {
  const int st = contrast_nhwc_args_ok(dtype, g, B, HW, ld, C, header, idx_b, idx_p, cap, N, n_match, dA, A, norms);
  if (st != CAVP_OK) return st;
  const int rows = header ? cap : N;
  cavp_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    contrast_rows_bwd_add_kernel<T><<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>((T*)g, B, HW, ld, C, header, idx_b, idx_p, cap, N,
                                                                                    n_match, dA, A, norms, scale);
  });
  CHECK_LAUNCH();
}
