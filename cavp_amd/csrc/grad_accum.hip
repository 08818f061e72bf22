// Gradient accumulation for gfx950: N micro-batches per optimiser update, inside the captured step.
//
// A window of n micro-steps sums their gradients element by element in f32, in micro-step order, which is what torch's .grad
// accumulation does over n calls of (loss / n).backward().  The accumulator is a second flat f32 buffer with the gradient arena's
// layout; an element of it lives at its gradient's offset from the arena's base.  With g the arena after micro-step k:
//   k == 0          acc <- g          a copy: the accumulator is neither read nor zeroed, so nothing of an earlier window survives
//   0 < k < n - 1   acc <- acc + g
//   k == n - 1      g   <- acc + g    the window's sum goes back INTO THE ARENA, where the guard, the update and p.grad read it
//   n == 1          nothing
// k and n come from the device-resident cavp_accum_state: uniform over a launch, so no divergence, and the launch takes nothing
// from the host - it can be recorded in a hipGraph and every replay runs the next micro-step.  cavp_grad_accumulate only READS
// the state block (other workgroups of the same launch read it too); the one-thread cavp_accum_advance behind it on the stream
// sets the gate word of the gated optimiser launches (optimizer.hip), advances k, keeps the loss sums / window means and counts.
//
// The optimiser's job table and block map are reused: one 256-thread workgroup per 4096-element block, so gradients outside the
// table (parameters the optimiser does not update) and the padding between views are never touched.
// HBM-bound streaming: k == 0 is 1 read + 1 write of 4 bytes per element, later micro-steps are 2 reads + 1 write.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kElemsPerBlock = 4096;   // 256 threads x 4 float4: cavp_optimizer_blocks' block (checked at the entry point)

// binary search: last job with blk0 <= blockIdx.x (uniform per workgroup), as in optimizer.hip
__device__ __forceinline__ int job_of_block(const cavp_opt_job* __restrict__ jobs, int njobs) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Every element is touched once per launch and the two buffers are larger than the last-level cache, so all 16-byte accesses
// carry the nontemporal hint: measured on the model's arena it is worth 9 % on the copy and 18 % on the adds over plain
// loads and stores (gradient accumulation).
__device__ __forceinline__ f32x4_t ld4(const float* p) { return __builtin_nontemporal_load((const f32x4_t*)p); }
__device__ __forceinline__ void st4(float* p, f32x4_t v) { __builtin_nontemporal_store(v, (f32x4_t*)p); }

enum { kCopy = 0, kAdd = 1, kClose = 2 };

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                              const float* arena_base, float* acc_base,
                                                              const cavp_accum_state* __restrict__ state) {
  const int n = state->n, k = state->k;
  if (n <= 1) return;   // every update sees one micro-batch: the arena already holds the window
  const int mode = k <= 0 ? kCopy : (k < n - 1 ? kAdd : kClose);
  const cavp_opt_job J = jobs[job_of_block(jobs, njobs)];
  const long long base = (long long)(blockIdx.x - J.blk0) * kElemsPerBlock;
  float* g = const_cast<float*>(J.g);            // written only by the closing micro-step
  float* a = acc_base + (J.g - arena_base);      // the bases are 16-byte aligned, so a is aligned exactly where g is
  if (J.vec && base + kElemsPerBlock <= J.n) {   // a full block: every 16-byte load is in flight before the first add
    f32x4_t gv[4], av[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) gv[q] = ld4(g + base + (q * 256 + threadIdx.x) * 4ll);
    if (mode == kCopy) {
#pragma unroll
      for (int q = 0; q < 4; ++q) st4(a + base + (q * 256 + threadIdx.x) * 4ll, gv[q]);
      return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = ld4(a + base + (q * 256 + threadIdx.x) * 4ll);
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = av[q] + gv[q];
    float* out = mode == kClose ? g : a;
#pragma unroll
    for (int q = 0; q < 4; ++q) st4(out + base + (q * 256 + threadIdx.x) * 4ll, av[q]);
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long i = base + (q * 256 + threadIdx.x) * 4ll;
    if (i >= J.n) break;
    if (i + 4 <= J.n && J.vec) {
      const f32x4_t gv = ld4(g + i);
      if (mode == kCopy) {
        st4(a + i, gv);
      } else {
        st4((mode == kClose ? g : a) + i, ld4(a + i) + gv);
      }
    } else {   // tails and unaligned views: scalar loads and stores, nothing past the end
      for (long long e = i; e < i + 4 && e < J.n; ++e) {
        if (mode == kCopy) {
          a[e] = g[e];
        } else {
          const float s = a[e] + g[e];
          if (mode == kClose) g[e] = s; else a[e] = s;
        }
      }
    }
  }
}

// One thread, behind the accumulate launch on the stream: nothing of that launch is still reading k when this writes it.
// The window mean is sum / n rounded to f32 once: the quotient is formed in double, whose 53 bits are >= 2 * 24 + 2, so the second
// rounding cannot move the result off the correctly rounded f32 quotient, whatever the build's f32 division is.
__global__ void accum_advance_kernel(cavp_accum_state* state, const float* loss0, const float* loss1) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int n = state->n > 1 ? state->n : 1;
  int k = state->k;
  if (k < 0 || k >= n) k = 0;
  const int gate = k == n - 1;
  if (loss0) {
    const float s = k == 0 ? loss0[0] : state->loss_sum0 + loss0[0];
    state->loss_sum0 = s;
    if (gate) state->loss_mean0 = (float)((double)s / (double)n);
  }
  if (loss1) {
    const float s = k == 0 ? loss1[0] : state->loss_sum1 + loss1[0];
    state->loss_sum1 = s;
    if (gate) state->loss_mean1 = (float)((double)s / (double)n);
  }
  state->gate = gate;
  state->k = gate ? 0 : k + 1;
  state->windows += gate;
  state->micro_total += 1;
}

}  // namespace

extern "C" int64_t cavp_accum_state_bytes(void) { return (int64_t)sizeof(cavp_accum_state); }

extern "C" int cavp_grad_accumulate(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, const float* arena_base,
                                    float* acc_base, const cavp_accum_state* state_device, void* stream) {
  if (!jobs_device || !arena_base || !acc_base || !state_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  if (!al16(arena_base) || !al16(acc_base)) return CAVP_ERR_ALIGN;
  if (cavp_optimizer_blocks(kElemsPerBlock) != 1 || cavp_optimizer_blocks(kElemsPerBlock + 1) != 2) return CAVP_ERR_UNSUPPORTED;
  grad_accumulate_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, arena_base, acc_base, state_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_accum_advance(cavp_accum_state* state_device, const float* loss0, const float* loss1, void* stream) {
  if (!state_device) return CAVP_ERR_BAD_ARG;
  accum_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state_device, loss0, loss1);
  CHECK_LAUNCH();
}
