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
