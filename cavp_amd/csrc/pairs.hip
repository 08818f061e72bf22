// Mismatched audio-visual pairs on the device (include/cavp_hip.h, "pair builder"): the block in front of the model call of
// the reference trainers (trainer_cavp_vpo_mono.py:87-115,148-181 with SoundBank, models/cavp_model.py:21-52) as four launches
// with no host value that depends on a device value.  plan -> gather -> bank_update -> labels; the plan kernel turns the
// batch's image labels into two small tables, the other three are copies steered by them.
#include "host_util.h"

constexpr int kPairsMaxB = 1024;   // rows of a batch: one thread each in the plan kernel
constexpr int kPairsMaxK = 256;    // classes: one thread each for the ring heads

// (key, i) order of the draws: smaller key first, ties by the row
__device__ __forceinline__ bool pair_before(unsigned long long ka, int ia, unsigned long long kb, int ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// One workgroup, thread t = row t.  The O(B^2) rank / position counts read LDS words that every lane asks for at the same time
// (a broadcast), 1024 iterations at the largest batch: microseconds, and no second sort to get wrong.
__global__ __launch_bounds__(kPairsMaxB) void pairs_plan_kernel(const long long* __restrict__ img, int B, int K, int S,
                                                                const int* __restrict__ perm_in, const int* __restrict__ rank_in,
                                                                int overwrite, const int* __restrict__ ow_table,
                                                                long long* __restrict__ state, int* __restrict__ head,
                                                                int* __restrict__ header, int* __restrict__ perm,
                                                                unsigned char* __restrict__ if_match, long long* __restrict__ img_sh,
                                                                int* __restrict__ source, int* __restrict__ src_table,
                                                                int* __restrict__ wr_table) {
  __shared__ unsigned long long skey[kPairsMaxB];   // shuffle keys, sorted in place
  __shared__ unsigned long long rkey[kPairsMaxB];   // overwrite ranks
  __shared__ int sidx[kPairsMaxB];
  __shared__ int single[kPairsMaxB];                // the row's only non-background class; -1: none or several
  __shared__ unsigned char fls[kPairsMaxB];         // the shuffled clip does not match the frame
  __shared__ int shead[kPairsMaxK];                 // ring heads before this step
  __shared__ int s_bad, s_over, s_wr;
  const int t = threadIdx.x;
  const unsigned long long seed = (unsigned long long)state[0], off = (unsigned long long)state[1];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), o0 = (unsigned)off, o1 = (unsigned)(off >> 32);
  if (t == 0) { s_bad = 0; s_over = 0; s_wr = 0; }
  if (t < K) {
    const int h = head[t];
    shead[t] = (h >= 0 && h < S) ? h : 0;
  }
  __syncthreads();
  // ---- the permutation: perm[j] = the row with the j-th smallest (key, i); bitonic network over the next power of two, the
  // padding carries the largest key and an index past every row, so it sorts behind a real row that drew the same key
  if (!perm_in) {
    int n = 1;
    while (n < B) n <<= 1;
    if (t < n) {
      skey[t] = t < B ? philox_key((unsigned)t, 0u, o0, o1, k0, k1) : ~0ull;
      sidx[t] = t;
    }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        const int p = t ^ j;
        if (t < n && p > t) {
          const unsigned long long ka = skey[t], kb = skey[p];
          const int ia = sidx[t], ib = sidx[p];
          const bool ascending = (t & k) == 0;
          if (pair_before(kb, ib, ka, ia) == ascending) {
            skey[t] = kb; sidx[t] = ib;
            skey[p] = ka; sidx[p] = ia;
          }
        }
        __syncthreads();
      }
  }
  int pm = t;
  if (t < B) {
    pm = perm_in ? perm_in[t] : sidx[t];
    if (pm < 0 || pm >= B) {   // a caller's perm that is no row: counted, and replaced so that nothing reads out of bounds
      atomicAdd(&s_bad, 1);
      pm = t;
    }
    const long long* a = img + (size_t)t * K;
    const long long* b = img + (size_t)pm * K;
    int cnt = 0, cls = -1, bad = 0;
    bool eq = true;
    for (int c = 0; c < K; ++c) {
      const long long va = a[c];
      eq = eq && va == b[c];
      bad += (unsigned long long)va > 1ull;
      if (c > 0 && va != 0) { ++cnt; cls = c; }
    }
    single[t] = cnt == 1 ? cls : -1;
    fls[t] = eq ? 0 : 1;
    rkey[t] = rank_in ? (unsigned long long)(unsigned)rank_in[t] : philox_key((unsigned)t, 1u, o0, o1, k0, k1);
    if (bad) atomicAdd(&s_bad, bad);
  }
  __syncthreads();
  int n_false = 0, q = 0;
  if (t < B) {
    // ---- overwrite: the q mismatched rows with the smallest (rank, i); of those, the single-source ones take the bank's clip
    int before = 0;
    const unsigned long long mykey = rkey[t];
    for (int j = 0; j < B; ++j)
      if (fls[j]) {
        ++n_false;
        before += pair_before(rkey[j], j, mykey, t);
      }
    q = overwrite ? ow_table[n_false] : 0;
    const int c = single[t];
    const bool ow = fls[t] && before < q && c >= 0;
    perm[t] = pm;
    if_match[t] = (!fls[t] || ow) ? 1 : 0;
    const long long* from = img + (size_t)(ow ? t : pm) * K;
    for (int k = 0; k < K; ++k) img_sh[(size_t)t * K + k] = from[k];
    source[t] = ow ? ~c : pm;
    src_table[t] = t;
    src_table[B + t] = ow ? ~(c * S + shead[c]) : pm;   // logical slot 0 = the physical slot at the head
    // ---- bank push: row t is the p-th of n_c single-source rows of class c; push p lands in physical (head + p) % S, and a
    // push that S later ones of the same batch would push out again is not written at all: no two writers share a slot
    int w = -1;
    if (c >= 0) {
      int p = 0, nc = 0;
      for (int j = 0; j < B; ++j)
        if (single[j] == c) {
          ++nc;
          p += j < t;
        }
      if (p >= nc - S) w = c * S + (shead[c] + p) % S;
    }
    wr_table[t] = w;
    if (ow) atomicAdd(&s_over, 1);
    if (w >= 0) atomicAdd(&s_wr, 1);
  }
  __syncthreads();
  if (t < K) {   // every reader used the LDS copy: the heads can move now
    int nc = 0;
    for (int j = 0; j < B; ++j) nc += single[j] == t;
    if (nc) head[t] = (shead[t] + nc) % S;
  }
  if (t == 0) {
    header[0] = n_false;
    header[1] = q;
    header[2] = s_over;
    header[3] = s_wr;
    header[4] = (int)o0;
    header[5] = (int)o1;
    header[6] = (int)k0;
    header[7] = (int)k1;
    state[1] = (long long)(off + 1ull);
    state[2] += s_bad;
  }
}

// dst[0 .. n) = src[0 .. n) by the workgroups of one grid row (blockIdx.x strides the row); VEC: 16 bytes per access
template <typename V>
__device__ __forceinline__ void pairs_copy_row(const V* __restrict__ src, V* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

// out row r = waveform row e (e >= 0) or bank slot ~e (e < 0), e = src_table[r]
template <bool VEC>
__global__ __launch_bounds__(256) void pairs_gather_kernel(const float* __restrict__ wave, const float* __restrict__ bank,
                                                           const int* __restrict__ src_table, int B, int nslots, int A,
                                                           float* __restrict__ out) {
  const int r = blockIdx.y, e = src_table[r];
  const float* src;
  if (e >= 0) {
    if (e >= B) return;
    src = wave + (size_t)e * A;
  } else {
    if (~e >= nslots) return;
    src = bank + (size_t)(~e) * A;
  }
  float* dst = out + (size_t)r * A;
  if (VEC)
    pairs_copy_row((const float4*)src, (float4*)dst, A >> 2);
  else
    pairs_copy_row(src, dst, A);
}

// bank slot wr_table[r] = waveform row r for the writer rows (wr_table[r] >= 0)
template <bool VEC>
__global__ __launch_bounds__(256) void pairs_bank_update_kernel(const float* __restrict__ wave, const int* __restrict__ wr_table,
                                                                int nslots, int A, float* __restrict__ bank) {
  const int r = blockIdx.y, w = wr_table[r];
  if (w < 0 || w >= nslots) return;
  const float* src = wave + (size_t)r * A;
  float* dst = bank + (size_t)w * A;
  if (VEC)
    pairs_copy_row((const float4*)src, (float4*)dst, A >> 2);
  else
    pairs_copy_row(src, dst, A);
}

// label_shuffle row r = pix_label row r where the pair matches, background (0) where it does not - written without a read
template <bool VEC>
__global__ __launch_bounds__(256) void pairs_labels_kernel(const long long* __restrict__ pix, const unsigned char* __restrict__ if_match,
                                                           long long HW, long long* __restrict__ out) {
  const int r = blockIdx.y;
  const long long* src = pix + (size_t)r * HW;
  long long* dst = out + (size_t)r * HW;
  if (if_match[r]) {
    if (VEC)
      pairs_copy_row((const uint4*)src, (uint4*)dst, HW >> 1);
    else
      pairs_copy_row(src, dst, HW);
  } else if (VEC) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (HW >> 1); i += (long long)gridDim.x * 256) ((uint4*)dst)[i] = z;
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) dst[i] = 0;
  }
}

// workgroups per row: 256 threads x 4 accesses each, at most 64 per row
static inline unsigned pairs_row_blocks(long long accesses) {
  long long nb = (accesses + 1023) / 1024;
  return (unsigned)(nb < 1 ? 1 : nb > 64 ? 64 : nb);
}

extern "C" int cavp_pairs_plan(const int64_t* img_label, int32_t B, int32_t K, int32_t S, const int32_t* perm_in,
                               const int32_t* rank_in, int32_t overwrite, const int32_t* ow_table, int32_t ow_table_len,
                               int64_t* state, int32_t* head, int32_t* header, int32_t* perm, uint8_t* if_match,
                               int64_t* img_label_shuffle, int32_t* source, int32_t* src_table, int32_t* wr_table, void* stream) {
  if (!img_label || !ow_table || !state || !head || !header || !perm || !if_match || !img_label_shuffle || !source || !src_table ||
      !wr_table)
    return CAVP_ERR_BAD_ARG;
  if (B < 1 || K < 1 || S < 1 || ow_table_len <= B) return CAVP_ERR_BAD_ARG;
  if (B > kPairsMaxB || K > kPairsMaxK || (long long)K * S > 0x7fffffffll) return CAVP_ERR_UNSUPPORTED;
  pairs_plan_kernel<<<1, kPairsMaxB, 0, (hipStream_t)stream>>>((const long long*)img_label, B, K, S, perm_in, rank_in, overwrite ? 1 : 0,
                                                               ow_table, (long long*)state, head, header, perm, if_match,
                                                               (long long*)img_label_shuffle, source, src_table, wr_table);
  CHECK_LAUNCH();
}

extern "C" int cavp_pairs_gather(const float* waveform, const float* bank, const int32_t* src_table, int32_t B, int32_t K, int32_t S,
                                 int32_t A, float* out, void* stream) {
  if (!waveform || !bank || !src_table || !out || B < 1 || K < 1 || S < 1 || A < 1) return CAVP_ERR_BAD_ARG;
  if (B > kPairsMaxB || K > kPairsMaxK || (long long)K * S > 0x7fffffffll) return CAVP_ERR_UNSUPPORTED;
  const bool vec = A % 4 == 0 && al16(waveform) && al16(bank) && al16(out);
  const dim3 grid(pairs_row_blocks(vec ? A / 4 : A), 2 * B);
  if (vec)
    pairs_gather_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(waveform, bank, src_table, B, K * S, A, out);
  else
    pairs_gather_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(waveform, bank, src_table, B, K * S, A, out);
  CHECK_LAUNCH();
}

extern "C" int cavp_pairs_bank_update(const float* waveform, const int32_t* wr_table, int32_t B, int32_t K, int32_t S, int32_t A,
                                      float* bank, void* stream) {
  if (!waveform || !bank || !wr_table || B < 1 || K < 1 || S < 1 || A < 1) return CAVP_ERR_BAD_ARG;
  if (B > kPairsMaxB || K > kPairsMaxK || (long long)K * S > 0x7fffffffll) return CAVP_ERR_UNSUPPORTED;
  const bool vec = A % 4 == 0 && al16(waveform) && al16(bank);
  const dim3 grid(pairs_row_blocks(vec ? A / 4 : A), B);
  if (vec)
    pairs_bank_update_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(waveform, wr_table, K * S, A, bank);
  else
    pairs_bank_update_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(waveform, wr_table, K * S, A, bank);
  CHECK_LAUNCH();
}

extern "C" int cavp_pairs_labels(const int64_t* pix_label, const uint8_t* if_match, int32_t B, int64_t HW, int64_t* label_shuffle,
                                 void* stream) {
  if (!pix_label || !if_match || !label_shuffle || B < 1 || HW < 1) return CAVP_ERR_BAD_ARG;
  if (B > kPairsMaxB) return CAVP_ERR_UNSUPPORTED;
  const bool vec = HW % 2 == 0 && al16(pix_label) && al16(label_shuffle);
  const dim3 grid(pairs_row_blocks(vec ? HW / 2 : HW), B);
  if (vec)
    pairs_labels_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>((const long long*)pix_label, if_match, HW, (long long*)label_shuffle);
  else
    pairs_labels_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>((const long long*)pix_label, if_match, HW, (long long*)label_shuffle);
  CHECK_LAUNCH();
}
