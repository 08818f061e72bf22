// Resident data set: the epoch sampler and the batch gather on the device (include/cavp_hip.h, "device store").  Two launches
// with no host value that depends on a device value: plan (one workgroup: the B item indices of step t by a keyed Feistel
// permutation, the per-row table, t + 1) -> gather (ragged byte rows from the three arenas into the staging buffers that
// FrameAugment and WaveStage read).
#include <algorithm>

#include "host_util.h"

constexpr int kStoreMaxB = 1024;      // rows of a batch: one thread each in the plan kernel
constexpr int kStoreRounds = 8;       // Feistel rounds
constexpr int kStoreChunkVec = 256;   // 16-byte vectors one wave moves per work item: 4 per lane, 4 KiB

// pi_e(x) on [0, N): a balanced Feistel network on 2k bits, round function = the first Philox word at counter (R, r, e_lo, e_hi),
// re-applied until the value is below N (cycle walking: the network is a bijection of [0, 2^2k) and 2^2k < 4N, so the walk
// comes back into [0, N) and its expected length is below 4)
__device__ __forceinline__ unsigned store_permute(unsigned x, unsigned N, int k, unsigned e0, unsigned e1, unsigned k0, unsigned k1) {
  const unsigned mask = (1u << k) - 1u;
  do {
    unsigned L = x >> k, R = x & mask;
#pragma unroll 1
    for (unsigned r = 0; r < (unsigned)kStoreRounds; ++r) {
      const unsigned f = (unsigned)(philox_key(R, r, e0, e1, k0, k1) >> 32);
      const unsigned nr = L ^ (f & mask);
      L = R;
      R = nr;
    }
    x = (L << k) | R;
  } while (x >= N);
  return x;
}

// plan row b: int64 [4 + 3 * S] = {frame_off, mask_off, h, w, then per source {pcm_off, length, n_ch}} - byte offsets into the
// arenas; an absent source has length = n_ch = 0
__global__ __launch_bounds__(kStoreMaxB) void store_plan_kernel(
    const long long* __restrict__ frame_off, const long long* __restrict__ mask_off, const int* __restrict__ size,
    const int* __restrict__ n_src, const long long* __restrict__ pcm_off, const int* __restrict__ length,
    const int* __restrict__ rate_idx, const int* __restrict__ n_ch, long long frame_bytes, long long mask_bytes, long long pcm_bytes,
    int N, int B, int S, int Hs, int Ws, int Cm, long long Lmax, int elem, int rank, int world, int kbits,
    const int* __restrict__ index_in, long long* __restrict__ state, int* __restrict__ out_index, int* __restrict__ out_sizes,
    int* __restrict__ out_length, int* __restrict__ out_rate, int* __restrict__ out_nch, long long* __restrict__ plan) {
  __shared__ int s_bad;
  const int i = threadIdx.x;
  const unsigned long long seed = (unsigned long long)state[0];
  const long long t = state[1];
  if (i == 0) s_bad = 0;
  __syncthreads();   // every thread has read t before thread 0 moves it
  if (i < B) {
    int bad = 0, item;
    if (index_in) {
      item = index_in[i];
      if (item < 0 || item >= N) {   // counted, and replaced so that nothing reads out of bounds
        ++bad;
        item = 0;
      }
    } else {
      const long long M = ((long long)N + world - 1) / world, spe = M / B;   // items per rank, steps per epoch (drop_last)
      const unsigned long long tt = (unsigned long long)t, e = tt / (unsigned long long)spe;
      const long long j = (long long)(tt - e * (unsigned long long)spe) * B + i;
      long long q = j * world + rank;
      if (q >= N) q -= N;            // DistributedSampler's wrap-around padding (j < M, so q < M * world < N + world <= 2N)
      item = (int)store_permute((unsigned)q, (unsigned)N, kbits, (unsigned)e, (unsigned)(e >> 32), (unsigned)seed,
                                (unsigned)(seed >> 32));
    }
    // the tables come from DeviceStore.freeze(); they are checked all the same, and a piece that does not fit is left out
    long long* row = plan + (size_t)i * (4 + 3 * S);
    int h = size[2 * item], w = size[2 * item + 1];
    const long long fo = frame_off[item], mo = mask_off[item];
    if (h < 1 || h > Hs || w < 1 || w > Ws || fo < 0 || fo + 3ll * h * w > frame_bytes || mo < 0 || mo + (long long)h * w > mask_bytes) {
      ++bad;
      h = w = 0;
    }
    row[0] = fo;
    row[1] = mo;
    row[2] = h;
    row[3] = w;
    out_index[i] = item;
    out_sizes[2 * i] = h;
    out_sizes[2 * i + 1] = w;
    int ns = n_src[item];
    if (ns < 0 || ns > S) {
      ++bad;
      ns = 0;
    }
    for (int s = 0; s < S; ++s) {
      long long po = 0;
      int len = 0, nc = 0;
      if (s < ns) {
        po = pcm_off[(size_t)item * S + s];
        len = length[(size_t)item * S + s];
        nc = n_ch[(size_t)item * S + s];
        if (len < 1 || len > Lmax || nc < 1 || nc > Cm || po < 0 || po + (long long)nc * len * elem > pcm_bytes) {
          ++bad;
          len = nc = 0;
        } else {
          out_rate[(size_t)i * S + s] = rate_idx[(size_t)item * S + s];
        }
      }
      row[4 + 3 * s] = po;
      row[5 + 3 * s] = len;
      row[6 + 3 * s] = nc;
      out_length[(size_t)i * S + s] = len;
      out_nch[(size_t)i * S + s] = nc;
    }
    if (bad) atomicAdd(&s_bad, bad);
  }
  __syncthreads();
  if (i == 0) {
    state[1] = t + 1;
    state[2] += s_bad;
  }
}

// 16 bytes from any byte address (the hardware takes unaligned global loads; the compiler emits one global_load_dwordx4)
__device__ __forceinline__ uint4 store_load16(const unsigned char* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// `rows` rows of `n` bytes, back to back at src, dst_stride apart at dst, by the `nw` waves of one grid segment (this wave: gw).
// Per row: head = the bytes up to dst's 16-byte boundary, body = 16-byte stores fed by unaligned 16-byte loads, tail = the rest;
// every load and every store lies inside the row.  Work item = (row, chunk of 256 body vectors); chunk 0 also moves head and tail.
__device__ __forceinline__ void store_copy_rows(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, unsigned rows,
                                                long long n, long long dst_stride, unsigned gw, unsigned nw) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned cpr = (unsigned)((n >> 4) / kStoreChunkVec) + 1u;   // chunks per row (the body has n / 16 or n / 16 - 1 vectors)
  const unsigned total = rows * cpr;
  for (unsigned it = gw; it < total; it += nw) {
    const unsigned r = it / cpr, c = it - r * cpr;
    const unsigned char* s = src + (size_t)r * n;
    unsigned char* d = dst + (size_t)r * dst_stride;
    long long head = (long long)((16u - (unsigned)((uintptr_t)d & 15u)) & 15u);
    if (head > n) head = n;
    const long long nb = (n - head) >> 4;
    const long long v0 = (long long)c * kStoreChunkVec + lane;
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v0 + 64 * k < nb) v[k] = store_load16(s + head + 16 * (v0 + 64 * k));
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v0 + 64 * k < nb) *(uint4*)(d + head + 16 * (v0 + 64 * k)) = v[k];
    if (c == 0) {
      const long long tail0 = head + 16 * nb;
      if ((long long)lane < head) d[lane] = s[lane];
      if (lane >= 16 && tail0 + (lane - 16) < n) d[tail0 + (lane - 16)] = s[tail0 + (lane - 16)];   // (lanes 16 .. 30: n - tail0 <= 15)
    }
  }
}

// grid (x, B, 2 + S * Cm): segment z = 0 the frame of row b, 1 its mask, 2 + s * Cm + c channel c of source s
__global__ __launch_bounds__(256) void store_gather_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ masks,
                                                           const unsigned char* __restrict__ pcm, const long long* __restrict__ plan,
                                                           int S, int Hs, int Ws, int Cm, long long Lmax, int elem,
                                                           unsigned char* __restrict__ out_frames, unsigned char* __restrict__ out_masks,
                                                           unsigned char* __restrict__ out_pcm) {
  const int b = blockIdx.y, z = blockIdx.z;
  const long long* row = plan + (size_t)b * (4 + 3 * S);
  const unsigned gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), nw = gridDim.x * 4;
  if (z < 2) {
    const int h = (int)row[2], w = (int)row[3];
    if (h < 1 || w < 1 || h > Hs || w > Ws) return;
    const int px = z == 0 ? 3 : 1;
    const unsigned char* src = (z == 0 ? frames : masks) + row[z];
    unsigned char* dst = (z == 0 ? out_frames : out_masks) + (size_t)b * Hs * Ws * px;
    if (w == Ws)   // the window spans whole staging rows: one row of h * w pixels
      store_copy_rows(src, dst, 1u, (long long)h * w * px, 0, gw, nw);
    else
      store_copy_rows(src, dst, (unsigned)h, (long long)w * px, (long long)Ws * px, gw, nw);
  } else {
    const int s = (z - 2) / Cm, c = (z - 2) - s * Cm;
    const long long len = row[5 + 3 * s];
    const int nc = (int)row[6 + 3 * s];
    if (c >= nc || len < 1 || len > Lmax) return;
    const unsigned char* src = pcm + row[4 + 3 * s] + (size_t)c * len * elem;
    unsigned char* dst = out_pcm + (((size_t)b * S + s) * Cm + c) * (size_t)Lmax * elem;
    store_copy_rows(src, dst, 1u, len * elem, 0, gw, nw);
  }
}

static inline bool store_dims_ok(int B, int S, int Hs, int Ws, int Cm, long long Lmax, int elem) {
  return B >= 1 && S >= 1 && Hs >= 1 && Ws >= 1 && Cm >= 1 && Lmax >= 1 && (elem == 2 || elem == 4);
}
static inline bool store_dims_supported(int B, int S, int Hs, int Ws, int Cm, long long Lmax) {
  return B <= kStoreMaxB && Hs <= CAVP_STORE_MAX_STAGE && Ws <= CAVP_STORE_MAX_STAGE && Lmax <= (1ll << 28) &&
         2ll + (long long)S * Cm <= 65535;
}

extern "C" int cavp_store_plan_words(int32_t S) { return 4 + 3 * S; }

extern "C" int cavp_store_plan(const int64_t* frame_off, const int64_t* mask_off, const int32_t* size, const int32_t* n_src,
                               const int64_t* pcm_off, const int32_t* length, const int32_t* rate_idx, const int32_t* n_ch,
                               int64_t frame_bytes, int64_t mask_bytes, int64_t pcm_bytes, int32_t N, int32_t B, int32_t S, int32_t Hs,
                               int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem, int32_t rank, int32_t world, const int32_t* index_in,
                               int64_t* state, int32_t* out_index, int32_t* out_sizes, int32_t* out_length, int32_t* out_rate_idx,
                               int32_t* out_n_ch, int64_t* plan, void* stream) {
  if (!frame_off || !mask_off || !size || !n_src || !pcm_off || !length || !rate_idx || !n_ch || !state || !out_index || !out_sizes ||
      !out_length || !out_rate_idx || !out_n_ch || !plan)
    return CAVP_ERR_BAD_ARG;
  if (!store_dims_ok(B, S, Hs, Ws, Cm, Lmax, elem) || N < 1 || world < 1 || rank < 0 || rank >= world || frame_bytes < 0 ||
      mask_bytes < 0 || pcm_bytes < 0)
    return CAVP_ERR_BAD_ARG;
  if (world > N || ((long long)N + world - 1) / world < B) return CAVP_ERR_BAD_ARG;   // no full batch in an epoch
  if (!store_dims_supported(B, S, Hs, Ws, Cm, Lmax)) return CAVP_ERR_UNSUPPORTED;
  int bits = 0;
  while (bits < 31 && (1ll << bits) < N) ++bits;   // bit_length(N - 1)
  if (bits < 2) bits = 2;
  store_plan_kernel<<<1, kStoreMaxB, 0, (hipStream_t)stream>>>(
      (const long long*)frame_off, (const long long*)mask_off, size, n_src, (const long long*)pcm_off, length, rate_idx, n_ch,
      frame_bytes, mask_bytes, pcm_bytes, N, B, S, Hs, Ws, Cm, Lmax, elem, rank, world, (bits + 1) / 2, index_in, (long long*)state,
      out_index, out_sizes, out_length, out_rate_idx, out_n_ch, (long long*)plan);
  CHECK_LAUNCH();
}

extern "C" int cavp_store_gather(const uint8_t* frames, const uint8_t* masks, const uint8_t* pcm, const int64_t* plan, int32_t B,
                                 int32_t S, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem, uint8_t* out_frames,
                                 uint8_t* out_masks, uint8_t* out_pcm, void* stream) {
  if (!frames || !masks || !pcm || !plan || !out_frames || !out_masks || !out_pcm) return CAVP_ERR_BAD_ARG;
  if (!store_dims_ok(B, S, Hs, Ws, Cm, Lmax, elem)) return CAVP_ERR_BAD_ARG;
  if (!store_dims_supported(B, S, Hs, Ws, Cm, Lmax)) return CAVP_ERR_UNSUPPORTED;
  // workgroups per segment: one per 32 KiB of the largest segment (two 4 KiB items for each of its four waves), at most 32
  const long long big = std::max<long long>(3ll * Hs * Ws, (long long)Lmax * elem);
  const long long gx = std::min(32ll, std::max(1ll, (big + 32767) / 32768));
  store_gather_kernel<<<dim3((unsigned)gx, (unsigned)B, (unsigned)(2 + S * Cm)), 256, 0, (hipStream_t)stream>>>(
      frames, masks, pcm, (const long long*)plan, S, Hs, Ws, Cm, Lmax, elem, out_frames, out_masks, out_pcm);
  CHECK_LAUNCH();
}

// ---- Clip store (include/cavp_hip.h, "clip store"): items are clips of up to 32 frames; the train plan draws one frame per row, the
// eval plan walks the clips in order and feeds every frame slot; one gather kernel serves both ----
constexpr int kClipMaxT = 32;
constexpr unsigned kClipDrawTag = 0xC11Fu;   // c1 of the frame draw's Philox counter (a Feistel counter has c1 < 8)

struct ClipTables {
  const long long *frame_off, *mask_off;   // [F]
  const int* size;                         // [F][2]
  const int *first, *n_frames;             // [N]
  const unsigned* avail;                   // [N]
  const int *mask_num, *tag, *n_src;       // [N]
  const long long* pcm_off;                // [N][S]
  const int *length, *rate_idx, *n_ch;     // [N][S]
  long long frame_bytes, mask_bytes, pcm_bytes, Lmax;
  int F, N, S, Tmax, Hs, Ws, Cm, elem;
};

// the clip's frame range, checked: 1 <= n <= Tmax and [first, first + n) inside the frame tables
__device__ __forceinline__ bool clip_head(const ClipTables& T, int clip, int& first, int& n) {
  first = T.first[clip];
  n = T.n_frames[clip];
  if (n < 1 || n > T.Tmax || first < 0 || (long long)first + n > T.F) {
    first = n = 0;
    return false;
  }
  return true;
}

// frame f of the frame tables, checked; mo = -1: no mask (an error where the caller needs one).  Not ok: an empty slot
__device__ __forceinline__ bool clip_frame(const ClipTables& T, int f, bool need_mask, long long& fo, long long& mo, int& h, int& w) {
  h = T.size[2 * f];
  w = T.size[2 * f + 1];
  fo = T.frame_off[f];
  mo = T.mask_off[f];
  const bool mask_ok = mo == -1 ? !need_mask : (mo >= 0 && mo + (long long)h * w <= T.mask_bytes);
  if (h < 1 || h > T.Hs || w < 1 || w > T.Ws || fo < 0 || fo + 3ll * h * w > T.frame_bytes || !mask_ok) {
    h = w = 0;
    fo = 0;
    mo = -1;
    return false;
  }
  return true;
}

// the PCM part of plan row `i` (src: its 3 S words) and of the tables, as in store_plan_kernel; returns the pieces left out
__device__ __forceinline__ int clip_sources(const ClipTables& T, int clip, int i, long long* __restrict__ src, int* __restrict__ out_length,
                                            int* __restrict__ out_rate, int* __restrict__ out_nch) {
  const int S = T.S;
  int bad = 0, ns = T.n_src[clip];
  if (ns < 0 || ns > S) {
    ++bad;
    ns = 0;
  }
  for (int s = 0; s < S; ++s) {
    long long po = 0;
    int len = 0, nc = 0;
    if (s < ns) {
      po = T.pcm_off[(size_t)clip * S + s];
      len = T.length[(size_t)clip * S + s];
      nc = T.n_ch[(size_t)clip * S + s];
      if (len < 1 || len > T.Lmax || nc < 1 || nc > T.Cm || po < 0 || po + (long long)nc * len * T.elem > T.pcm_bytes) {
        ++bad;
        po = 0;
        len = nc = 0;
      } else {
        out_rate[(size_t)i * S + s] = T.rate_idx[(size_t)clip * S + s];
      }
    }
    src[3 * s] = po;
    src[3 * s + 1] = len;
    src[3 * s + 2] = nc;
    out_length[(size_t)i * S + s] = len;
    out_nch[(size_t)i * S + s] = nc;
  }
  return bad;
}

// plan row i (T_out = 1): int64 [4 + 3 S] = {frame_off, mask_off, h, w, then per source {pcm_off, length, n_ch}}
__global__ __launch_bounds__(kStoreMaxB) void clips_plan_train_kernel(ClipTables T, int B, int rank, int world, int kbits,
                                                                      const int* __restrict__ index_in, const int* __restrict__ frame_in,
                                                                      long long* __restrict__ state, int* __restrict__ out_index,
                                                                      int* __restrict__ out_select, int* __restrict__ out_tag,
                                                                      int* __restrict__ out_sizes, int* __restrict__ out_length,
                                                                      int* __restrict__ out_rate, int* __restrict__ out_nch,
                                                                      long long* __restrict__ plan) {
  __shared__ int s_bad;
  const int i = threadIdx.x, N = T.N;
  const unsigned long long seed = (unsigned long long)state[0];
  const long long t = state[1];
  if (i == 0) s_bad = 0;
  __syncthreads();   // every thread has read t before thread 0 moves it
  if (i < B) {
    int bad = 0, clip;
    if (index_in) {
      clip = index_in[i];
      if (clip < 0 || clip >= N) {
        ++bad;
        clip = 0;
      }
    } else {
      const long long M = ((long long)N + world - 1) / world, spe = M / B;
      const unsigned long long tt = (unsigned long long)t, e = tt / (unsigned long long)spe;
      const long long j = (long long)(tt - e * (unsigned long long)spe) * B + i;
      long long q = j * world + rank;
      if (q >= N) q -= N;
      clip = (int)store_permute((unsigned)q, (unsigned)N, kbits, (unsigned)e, (unsigned)(e >> 32), (unsigned)seed,
                                (unsigned)(seed >> 32));
    }
    int first, n, fr = 0, h = 0, w = 0;
    long long fo = 0, mo = -1;
    bool ok = clip_head(T, clip, first, n);
    const unsigned av = ok ? T.avail[clip] : 0u;
    if (ok && (av == 0u || (n < 32 && (av >> n) != 0u))) ok = false;   // nothing to draw, or a bit beyond the clip
    if (!ok) ++bad;
    if (ok) {
      if (frame_in) {
        fr = frame_in[i];
        if (fr < 0 || fr >= kClipMaxT || !((av >> fr) & 1u)) {   // counted, and replaced by the lowest frame a draw may take
          ++bad;
          fr = __ffs((int)av) - 1;
        }
      } else {
        const unsigned word = (unsigned)(philox_key((unsigned)i, kClipDrawTag, (unsigned)(unsigned long long)t,
                                                    (unsigned)((unsigned long long)t >> 32), (unsigned)seed, (unsigned)(seed >> 32)) >> 32);
        const unsigned r = (unsigned)(((unsigned long long)word * (unsigned)__popc(av)) >> 32);
        unsigned m = av;
        for (unsigned k = 0; k < r; ++k) m &= m - 1u;   // drop the r lowest set bits
        fr = __ffs((int)m) - 1;
      }
      if (!clip_frame(T, first + fr, true, fo, mo, h, w)) ++bad;
    }
    long long* row = plan + (size_t)i * (4 + 3 * T.S);
    row[0] = fo;
    row[1] = mo;
    row[2] = h;
    row[3] = w;
    out_index[i] = clip;
    out_select[i] = fr;
    out_tag[i] = T.tag[clip];
    out_sizes[2 * i] = h;
    out_sizes[2 * i + 1] = w;
    bad += clip_sources(T, clip, i, row + 4, out_length, out_rate, out_nch);
    if (bad) atomicAdd(&s_bad, bad);
  }
  __syncthreads();
  if (i == 0) {
    state[1] = t + 1;
    state[2] += s_bad;
  }
}

// one thread per (row, frame slot); plan row i: int64 [4 Tmax + 3 S] = Tmax x {frame_off, mask_off, h, w}, then the sources
__global__ __launch_bounds__(kStoreMaxB) void clips_plan_eval_kernel(ClipTables T, int B, int rank, int world, long long P,
                                                                     long long* __restrict__ state, int* __restrict__ out_index,
                                                                     int* __restrict__ out_count, int* __restrict__ out_nframes,
                                                                     int* __restrict__ out_tag, int* __restrict__ out_sizes,
                                                                     int* __restrict__ out_length, int* __restrict__ out_rate,
                                                                     int* __restrict__ out_nch, long long* __restrict__ plan) {
  __shared__ int s_bad;
  const int Tm = T.Tmax, i = threadIdx.x / Tm, k = threadIdx.x - i * Tm;
  const long long t = state[3];
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  if (i < B) {
    const long long s = (long long)((unsigned long long)t % (unsigned long long)P);
    const long long q = (s * B + i) * world + rank;
    const bool pad = q >= T.N;
    const int clip = pad ? 0 : (int)q;
    int bad = 0, first, n, h = 0, w = 0, sh = 0, sw = 0;
    long long fo = 0, mo = -1;
    const bool ok = clip_head(T, clip, first, n);
    if (ok) {
      if (k < n) {
        if (!clip_frame(T, first + k, false, fo, mo, h, w)) ++bad;
        sh = h;
        sw = w;
      } else {   // no frame: nothing is copied, the size is frame 0's (whose own thread counts it if it is wrong)
        long long f0, m0;
        clip_frame(T, first, false, f0, m0, sh, sw);
      }
    }
    long long* row = plan + (size_t)i * (4 * Tm + 3 * T.S);
    row[4 * k] = fo;
    row[4 * k + 1] = mo;
    row[4 * k + 2] = h;
    row[4 * k + 3] = w;
    out_sizes[2 * ((size_t)i * Tm + k)] = sh;
    out_sizes[2 * ((size_t)i * Tm + k) + 1] = sw;
    if (k == 0) {
      int mn = ok ? T.mask_num[clip] : 0;
      if (!ok) ++bad;
      if (mn < 0 || mn > n) {
        ++bad;
        mn = 0;
      }
      out_index[i] = pad ? -1 : clip;
      out_count[i] = pad ? 0 : mn;
      out_nframes[i] = n;
      out_tag[i] = T.tag[clip];
      bad += clip_sources(T, clip, i, row + 4 * Tm, out_length, out_rate, out_nch);
    }
    if (bad) atomicAdd(&s_bad, bad);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    state[3] = t + 1;
    state[2] += s_bad;
  }
}

// grid (x, B, 2 T + S * Cm): segment z < T frame slot z of row b, z < 2 T mask slot z - T, then channel c of source s
__global__ __launch_bounds__(256) void clips_gather_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ masks,
                                                           const unsigned char* __restrict__ pcm, const long long* __restrict__ plan,
                                                           int T, int S, int Hs, int Ws, int Cm, long long Lmax, int elem,
                                                           unsigned char* __restrict__ out_frames, unsigned char* __restrict__ out_masks,
                                                           unsigned char* __restrict__ out_pcm) {
  const int b = blockIdx.y, z = blockIdx.z;
  const long long* row = plan + (size_t)b * (4 * T + 3 * S);
  const unsigned gw = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), nw = gridDim.x * 4;
  if (z < 2 * T) {
    const int is_mask = z >= T, k = z - is_mask * T;
    const long long* slot = row + 4 * k;
    const int h = (int)slot[2], w = (int)slot[3];
    const long long off = slot[is_mask];
    if (h < 1 || w < 1 || h > Hs || w > Ws || off < 0) return;   // no frame in the slot, or a frame without a mask
    const int px = is_mask ? 1 : 3;
    const unsigned char* src = (is_mask ? masks : frames) + off;
    unsigned char* dst = (is_mask ? out_masks : out_frames) + ((size_t)b * T + k) * Hs * Ws * px;
    if (w == Ws)
      store_copy_rows(src, dst, 1u, (long long)h * w * px, 0, gw, nw);
    else
      store_copy_rows(src, dst, (unsigned)h, (long long)w * px, (long long)Ws * px, gw, nw);
  } else {
    const int zz = z - 2 * T, s = zz / Cm, c = zz - s * Cm;
    const long long* src_row = row + 4 * T + 3 * s;
    const long long len = src_row[1];
    const int nc = (int)src_row[2];
    if (c >= nc || len < 1 || len > Lmax) return;
    const unsigned char* src = pcm + src_row[0] + (size_t)c * len * elem;
    unsigned char* dst = out_pcm + (((size_t)b * S + s) * Cm + c) * (size_t)Lmax * elem;
    store_copy_rows(src, dst, 1u, len * elem, 0, gw, nw);
  }
}

static inline bool clips_dims_supported(int B, int T, int S, int Hs, int Ws, int Cm, long long Lmax) {
  return B <= kStoreMaxB && Hs <= CAVP_STORE_MAX_STAGE && Ws <= CAVP_STORE_MAX_STAGE && Lmax <= (1ll << 28) &&
         2ll * T + (long long)S * Cm <= 65535;
}

extern "C" int cavp_clips_plan_words(int32_t T_out, int32_t S) { return 4 * T_out + 3 * S; }

#define CLIP_TABLES()                                                                                                          \
  ClipTables T{(const long long*)frame_off, (const long long*)mask_off, size, first, n_frames, avail, mask_num, tag, n_src,    \
               (const long long*)pcm_off, length, rate_idx, n_ch, frame_bytes, mask_bytes, pcm_bytes, Lmax, F, N, S, Tmax, Hs, \
               Ws, Cm, elem}

static inline int clips_tables_ok(const void* const* ptrs, int n, int64_t frame_bytes, int64_t mask_bytes, int64_t pcm_bytes, int F, int N,
                                  int B, int S, int Tmax, int Hs, int Ws, int Cm, long long Lmax, int elem, int rank, int world) {
  for (int k = 0; k < n; ++k)
    if (!ptrs[k]) return CAVP_ERR_BAD_ARG;
  if (!store_dims_ok(B, S, Hs, Ws, Cm, Lmax, elem) || N < 1 || F < N || Tmax < 1 || Tmax > kClipMaxT || world < 1 || rank < 0 ||
      rank >= world || world > N || frame_bytes < 0 || mask_bytes < 0 || pcm_bytes < 0)
    return CAVP_ERR_BAD_ARG;
  return CAVP_OK;
}

extern "C" int cavp_clips_plan_train(const int64_t* frame_off, const int64_t* mask_off, const int32_t* size, const int32_t* first,
                                     const int32_t* n_frames, const uint32_t* avail, const int32_t* mask_num, const int32_t* tag,
                                     const int32_t* n_src, const int64_t* pcm_off, const int32_t* length, const int32_t* rate_idx,
                                     const int32_t* n_ch, int64_t frame_bytes, int64_t mask_bytes, int64_t pcm_bytes, int32_t F, int32_t N,
                                     int32_t B, int32_t S, int32_t Tmax, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem,
                                     int32_t rank, int32_t world, const int32_t* index_in, const int32_t* frame_in, int64_t* state,
                                     int32_t* out_index, int32_t* out_select, int32_t* out_tag, int32_t* out_sizes, int32_t* out_length,
                                     int32_t* out_rate_idx, int32_t* out_n_ch, int64_t* plan, void* stream) {
  const void* ptrs[] = {frame_off, mask_off, size,  first,     n_frames,   avail,   mask_num,  tag,        n_src,        pcm_off,  length,
                        rate_idx,  n_ch,     state, out_index, out_select, out_tag, out_sizes, out_length, out_rate_idx, out_n_ch, plan};
  const int st = clips_tables_ok(ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), frame_bytes, mask_bytes, pcm_bytes, F, N, B, S, Tmax, Hs, Ws,
                                 Cm, Lmax, elem, rank, world);
  if (st != CAVP_OK) return st;
  if (((long long)N + world - 1) / world < B) return CAVP_ERR_BAD_ARG;   // no full batch in an epoch
  if (!clips_dims_supported(B, 1, S, Hs, Ws, Cm, Lmax)) return CAVP_ERR_UNSUPPORTED;
  int bits = 0;
  while (bits < 31 && (1ll << bits) < N) ++bits;
  if (bits < 2) bits = 2;
  CLIP_TABLES();
  clips_plan_train_kernel<<<1, kStoreMaxB, 0, (hipStream_t)stream>>>(T, B, rank, world, (bits + 1) / 2, index_in, frame_in,
                                                                     (long long*)state, out_index, out_select, out_tag, out_sizes,
                                                                     out_length, out_rate_idx, out_n_ch, (long long*)plan);
  CHECK_LAUNCH();
}

extern "C" int cavp_clips_plan_eval(const int64_t* frame_off, const int64_t* mask_off, const int32_t* size, const int32_t* first,
                                    const int32_t* n_frames, const uint32_t* avail, const int32_t* mask_num, const int32_t* tag,
                                    const int32_t* n_src, const int64_t* pcm_off, const int32_t* length, const int32_t* rate_idx,
                                    const int32_t* n_ch, int64_t frame_bytes, int64_t mask_bytes, int64_t pcm_bytes, int32_t F, int32_t N,
                                    int32_t B, int32_t S, int32_t Tmax, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem,
                                    int32_t rank, int32_t world, int64_t* state, int32_t* out_index, int32_t* out_count,
                                    int32_t* out_n_frames, int32_t* out_tag, int32_t* out_sizes, int32_t* out_length,
                                    int32_t* out_rate_idx, int32_t* out_n_ch, int64_t* plan, void* stream) {
  const void* ptrs[] = {frame_off, mask_off, size,  first,     n_frames,  avail,        mask_num, tag,       n_src,      pcm_off,      length,
                        rate_idx,  n_ch,     state, out_index, out_count, out_n_frames, out_tag,  out_sizes, out_length, out_rate_idx, out_n_ch,
                        plan};
  const int st = clips_tables_ok(ptrs, (int)(sizeof(ptrs) / sizeof(ptrs[0])), frame_bytes, mask_bytes, pcm_bytes, F, N, B, S, Tmax, Hs, Ws,
                                 Cm, Lmax, elem, rank, world);
  if (st != CAVP_OK) return st;
  if ((long long)B * Tmax > kStoreMaxB || !clips_dims_supported(B, Tmax, S, Hs, Ws, Cm, Lmax)) return CAVP_ERR_UNSUPPORTED;
  const long long M = ((long long)N + world - 1) / world, P = (M + B - 1) / B;
  CLIP_TABLES();
  clips_plan_eval_kernel<<<1, kStoreMaxB, 0, (hipStream_t)stream>>>(T, B, rank, world, P, (long long*)state, out_index, out_count,
                                                                    out_n_frames, out_tag, out_sizes, out_length, out_rate_idx, out_n_ch,
                                                                    (long long*)plan);
  CHECK_LAUNCH();
}

extern "C" int cavp_clips_gather(const uint8_t* frames, const uint8_t* masks, const uint8_t* pcm, const int64_t* plan, int32_t B,
                                 int32_t T_out, int32_t S, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem,
                                 uint8_t* out_frames, uint8_t* out_masks, uint8_t* out_pcm, void* stream) {
  if (!frames || !masks || !pcm || !plan || !out_frames || !out_masks || !out_pcm) return CAVP_ERR_BAD_ARG;
  if (!store_dims_ok(B, S, Hs, Ws, Cm, Lmax, elem) || T_out < 1 || T_out > kClipMaxT) return CAVP_ERR_BAD_ARG;
  if ((long long)B * T_out > kStoreMaxB || !clips_dims_supported(B, T_out, S, Hs, Ws, Cm, Lmax)) return CAVP_ERR_UNSUPPORTED;
  const long long big = std::max<long long>(3ll * Hs * Ws, (long long)Lmax * elem);
  const long long gx = std::min(32ll, std::max(1ll, (big + 32767) / 32768));
  clips_gather_kernel<<<dim3((unsigned)gx, (unsigned)B, (unsigned)(2 * T_out + S * Cm)), 256, 0, (hipStream_t)stream>>>(
      frames, masks, pcm, (const long long*)plan, T_out, S, Hs, Ws, Cm, Lmax, elem, out_frames, out_masks, out_pcm);
  CHECK_LAUNCH();
}
