// Step rollback for gfx950 (include/cavp_hip.h, "step rollback"): a device-resident table of byte ranges, one launch that copies
// every live range into its shadow (save) and one that copies the shadows back and zero-fills the scrub ranges (restore).  The
// restore reads one 32-bit word on the device first - the step guard's cavp_guard_state.skip - and every workgroup leaves after
// that load when it is clear, so the pair can sit in a captured iteration: a skipped step then also undoes what its forward wrote
// (BatchNorm running statistics and counters, the pair builder's sound bank and ring heads, the call counters of the samplers).
//
// Work units.  A range is cut into blocks of 1 KiB (one wave x 16 bytes) on a grid that starts at the 16-byte boundary at or below
// its live address; blk0 of the table is the running sum of those block counts, as cavp_opt_job.blk0 is for the optimiser.  A
// workgroup (4 waves) serves spans of 16 consecutive blocks = 16 KiB, whatever ranges they belong to: the 183 small ranges of the
// ResNet-50 model's BatchNorm state (231 KB) cost 20 workgroups, not one each, and a large range (the bank) is spread over the
// whole grid, which is capped at 2048 workgroups that stride over the spans.  HBM-bound streaming: one read + one write per byte.
//
// Copies are 16-byte vectors wherever the lane's vector lies inside the range and live and shadow share their offset from a
// 16-byte boundary (StepRollback lays its shadow arena out that way); heads, tails and ranges whose two offsets differ go dword
// by dword.  Plain vector loads and stores only; the only atomics are the two call counters.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kBlockBytes = 1024;   // one wave x 16 bytes
constexpr int kSpanBlocks = 16;     // blocks per workgroup pass: 4 waves x 4 vectors in flight
constexpr int kMaxGrid = 2048;      // 256 CUs x 8 workgroups; the rest is a stride loop

// binary search: last range with blk0 <= block (uniform per workgroup)
__device__ __forceinline__ int range_of_block(const cavp_rollback_range* __restrict__ tab, int n, int block) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].blk0 <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// kRestore false: live -> shadow, scrub ranges untouched.  kRestore true: shadow -> live and zeros into the scrub ranges, unless
// *word == 0 (word == nullptr: forced).
template <bool kRestore>
__global__ __launch_bounds__(256) void rollback_kernel(const cavp_rollback_range* __restrict__ tab, int n, int total_blocks,
                                                       const int32_t* __restrict__ word, cavp_rollback_state* __restrict__ state) {
  if constexpr (kRestore) {
    if (word != nullptr && word[0] == 0) return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    atomicAdd((unsigned long long*)(kRestore ? &state->restores : &state->saves), 1ull);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nspans = (total_blocks + kSpanBlocks - 1) / kSpanBlocks;
  for (int span = blockIdx.x; span < nspans; span += gridDim.x) {
    const int b0 = span * kSpanBlocks;
    int r = range_of_block(tab, n, b0);
    {
      // the whole span inside one range, clear of its head and tail, both sides on the same 16-byte grid: four loads in flight per
      // lane, then four stores, nothing per lane to decide
      const cavp_rollback_range R = tab[r];
      const long long a = (long long)((uintptr_t)R.live & 15);
      const long long v0 = (long long)(b0 - R.blk0) * kBlockBytes;
      const bool scrub = (R.flags & CAVP_ROLLBACK_SCRUB) != 0;
      const bool same = scrub || (((uintptr_t)R.live ^ (uintptr_t)R.shadow) & 15) == 0;
      if (same && v0 >= a && v0 + kSpanBlocks * kBlockBytes <= a + R.nbytes) {
        if (scrub && !kRestore) continue;
        // (named registers, not an array: the compiler placed a uint4[4] here in LDS)
        const int o = (wave * 64 + lane) * 16, step = 4 * 64 * 16;
        char* live = (char*)R.live - a + v0 + o;
        if (scrub) {
          const uint4 z = make_uint4(0u, 0u, 0u, 0u);
          *(uint4*)live = z;
          *(uint4*)(live + step) = z;
          *(uint4*)(live + 2 * step) = z;
          *(uint4*)(live + 3 * step) = z;
          continue;
        }
        char* shadow = (char*)R.shadow - a + v0 + o;
        const char* src = kRestore ? shadow : live;
        char* dst = kRestore ? live : shadow;
        const uint4 x0 = *(const uint4*)src, x1 = *(const uint4*)(src + step), x2 = *(const uint4*)(src + 2 * step),
                    x3 = *(const uint4*)(src + 3 * step);
        *(uint4*)dst = x0;
        *(uint4*)(dst + step) = x1;
        *(uint4*)(dst + 2 * step) = x2;
        *(uint4*)(dst + 3 * step) = x3;
        continue;
      }
    }
    // mixed span: every wave finds the range of each of its blocks by walking on from the span's first range (each range has at
    // least one block, so the walk is at most 15 steps per span).  All four loads of a lane are issued before its first store:
    // the small ranges of a model lie in hundreds of separate allocations, and a load that waits for its page must not hold the
    // next one back.  (Ranges do not overlap, so no store can feed a later load.)
    uint4 x[4];
    char* dst[4];
    unsigned inside[4];   // bit k: dword k of the lane's vector lies inside the range
    bool vec[4];          // ... all four do, and both sides are on the same 16-byte grid: one vector access
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      x[q] = make_uint4(0u, 0u, 0u, 0u);
      dst[q] = nullptr;
      inside[q] = 0u;
      vec[q] = false;
      const int b = b0 + q * 4 + wave;
      if (b >= total_blocks) continue;
      while (r + 1 < n && tab[r + 1].blk0 <= b) ++r;
      const cavp_rollback_range R = tab[r];
      const bool scrub = (R.flags & CAVP_ROLLBACK_SCRUB) != 0;
      if (scrub && !kRestore) continue;
      const long long a = (long long)((uintptr_t)R.live & 15);
      const long long lo = a, hi = a + R.nbytes;                               // the range on its virtual grid
      const long long v = (long long)(b - R.blk0) * kBlockBytes + lane * 16;   // this lane's vector on it
      if (v >= hi || v + 16 <= lo) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) inside[q] |= (v + 4 * k >= lo && v + 4 * k < hi) ? 1u << k : 0u;
      const bool same = scrub || (((uintptr_t)R.live ^ (uintptr_t)R.shadow) & 15) == 0;
      vec[q] = same && inside[q] == 0xFu;
      dst[q] = (char*)(kRestore ? R.live : R.shadow) - a + v;   // never dereferenced outside the range
      if (scrub) continue;
      const char* src = (const char*)(kRestore ? R.shadow : R.live) - a + v;
      if (vec[q]) {
        x[q] = *(const uint4*)src;
      } else {
        if (inside[q] & 1u) x[q].x = *(const uint32_t*)(src);
        if (inside[q] & 2u) x[q].y = *(const uint32_t*)(src + 4);
        if (inside[q] & 4u) x[q].z = *(const uint32_t*)(src + 8);
        if (inside[q] & 8u) x[q].w = *(const uint32_t*)(src + 12);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (inside[q] == 0u) continue;
      if (vec[q]) {
        *(uint4*)dst[q] = x[q];
      } else {
        if (inside[q] & 1u) *(uint32_t*)(dst[q]) = x[q].x;
        if (inside[q] & 2u) *(uint32_t*)(dst[q] + 4) = x[q].y;
        if (inside[q] & 4u) *(uint32_t*)(dst[q] + 8) = x[q].z;
        if (inside[q] & 8u) *(uint32_t*)(dst[q] + 12) = x[q].w;
      }
    }
  }
}

inline int rollback_grid(int total_blocks) {
  const int nspans = (total_blocks + kSpanBlocks - 1) / kSpanBlocks;
  return nspans < kMaxGrid ? nspans : kMaxGrid;
}

}  // namespace

extern "C" int64_t cavp_rollback_range_bytes(void) { return (int64_t)sizeof(cavp_rollback_range); }
extern "C" int64_t cavp_rollback_state_bytes(void) { return (int64_t)sizeof(cavp_rollback_state); }

extern "C" int64_t cavp_rollback_blocks(int64_t live_address, int64_t nbytes) {
  if (nbytes <= 0) return 0;
  return ((live_address & 15) + nbytes + kBlockBytes - 1) / kBlockBytes;
}

extern "C" int cavp_rollback_save(const cavp_rollback_range* table_device, int32_t nranges, int32_t total_blocks,
                                  cavp_rollback_state* state_device, void* stream) {
  if (nranges < 0 || total_blocks < 0) return CAVP_ERR_BAD_ARG;
  if (nranges == 0 || total_blocks == 0) return CAVP_OK;   // an empty table: nothing to do, nothing counted
  if (!table_device || !state_device) return CAVP_ERR_BAD_ARG;
  rollback_kernel<false><<<rollback_grid(total_blocks), 256, 0, (hipStream_t)stream>>>(table_device, nranges, total_blocks, nullptr,
                                                                                    state_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_rollback_restore(const cavp_rollback_range* table_device, int32_t nranges, int32_t total_blocks,
                                     const int32_t* word_device, cavp_rollback_state* state_device, void* stream) {
  if (nranges < 0 || total_blocks < 0) return CAVP_ERR_BAD_ARG;
  if (nranges == 0 || total_blocks == 0) return CAVP_OK;
  if (!table_device || !state_device) return CAVP_ERR_BAD_ARG;
  if (word_device && ((uintptr_t)word_device & 3)) return CAVP_ERR_ALIGN;
  rollback_kernel<true><<<rollback_grid(total_blocks), 256, 0, (hipStream_t)stream>>>(table_device, nranges, total_blocks,
                                                                                   word_device, state_device);
  CHECK_LAUNCH();
}
