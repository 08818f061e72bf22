// Fused multi-tensor optimiser step for gfx950: torch.optim.SGD(momentum, weight_decay) on the visual parameter groups and
// torch.optim.Adam on the audio encoder (reference main_vpo_mono.py:118-125), every parameter tensor of the model in ONE
// launch.  The job table (one entry per tensor: parameter, gradient view in the flat gradient arena, state buffers,
// group hyper-parameters) lives in device memory and is built once.  The per-step scalars (learning rate of the poly
// schedule, Adam bias corrections, the "first step" flag of the momentum buffer) come one of two ways:
//   * cavp_optimizer_step: kernel arguments computed by the host.  A captured launch of it keeps the learning rate and the
//     step count it was captured with for ever, so this entry point is for eager use;
//   * cavp_optimizer_schedule + cavp_optimizer_step_dev: a one-thread launch advances a device-resident cavp_opt_state (step
//     counter, warm-up + poly schedule of engine/lr_policy.py:30-43, bias corrections) and the update launch behind it on
//     the same stream loads the scalars from there.  Nothing is read or written by the host, so the pair can be recorded
//     in a hipGraph and every replay runs the next step of the schedule.
//
//   SGD  (torch.optim.SGD, dampening 0, nesterov False):  d = g + wd p;  buf = first ? d : mu buf + d;  p -= lr buf
//   Adam (torch.optim.Adam, amsgrad False, L2 weight decay):  d = g + wd p;  m = b1 m + (1-b1) d;  v = b2 v + (1-b2) d^2;
//        p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// HBM-bound streaming: 3 reads + 2 writes (SGD) / 4 reads + 3 writes (Adam) of 4 bytes per parameter.
#include "common.h"
#include "host_util.h"

namespace {

constexpr int kElemsPerBlock = 4096;   // 256 threads x 4 float4

// binary search: last job with blk0 <= blockIdx.x (uniform per workgroup)
__device__ __forceinline__ int job_of_block(const cavp_opt_job* __restrict__ jobs, int njobs) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the update of one workgroup's 4096 elements; shared by the kernels below, so equal scalars give equal bits.  kScale: the
// gradient is gscale * g (the step guard's clip coefficient), rounded to f32 in a statement of its own so that the products
// below contract exactly as they do without it: gscale == 1 gives the bits of the unscaled update.  This relies on the build's
// -ffp-contract=on (build.py), which contracts inside one expression only; hipcc's default (fast) contracts across statements
// and would fuse the scaling into g + wd p.
template <bool kScale>
__device__ __forceinline__ void optimizer_step_body(const cavp_opt_job* __restrict__ jobs, int njobs, float lr_sgd, float lr_adam,
                                                    float momentum, float beta1, float beta2, float eps, float bc1,
                                                    float bc2_sqrt, int first_step, float gscale = 1.f) {
  const cavp_opt_job J = jobs[job_of_block(jobs, njobs)];
  const long long base = (long long)(blockIdx.x - J.blk0) * kElemsPerBlock;
  const float wd = J.weight_decay;
  if (J.kind == 0) {
    const float lr = lr_sgd * J.lr_mult;
    for (int q = 0; q < 4; ++q) {
      const long long i = base + (q * 256 + threadIdx.x) * 4ll;
      if (i >= J.n) break;
      if (i + 4 <= J.n && J.vec) {
        float4 p = *(const float4*)(J.p + i);
        float4 g = *(const float4*)(J.g + i);
        if constexpr (kScale) {
          g.x *= gscale; g.y *= gscale; g.z *= gscale; g.w *= gscale;
        }
        float4 b = first_step ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)(J.m + i);
        const float d0 = g.x + wd * p.x, d1 = g.y + wd * p.y, d2 = g.z + wd * p.z, d3 = g.w + wd * p.w;
        b.x = first_step ? d0 : momentum * b.x + d0; b.y = first_step ? d1 : momentum * b.y + d1;
        b.z = first_step ? d2 : momentum * b.z + d2; b.w = first_step ? d3 : momentum * b.w + d3;
        p.x -= lr * b.x; p.y -= lr * b.y; p.z -= lr * b.z; p.w -= lr * b.w;
        *(float4*)(J.m + i) = b;
        *(float4*)(J.p + i) = p;
      } else {
        for (long long e = i; e < i + 4 && e < J.n; ++e) {
          float g = J.g[e];
          if constexpr (kScale) g *= gscale;
          const float d = g + wd * J.p[e];
          const float b = first_step ? d : momentum * J.m[e] + d;
          J.m[e] = b;
          J.p[e] -= lr * b;
        }
      }
    }
  } else {
    const float step = lr_adam * J.lr_mult / bc1;
    for (int q = 0; q < 4; ++q) {
      const long long i = base + (q * 256 + threadIdx.x) * 4ll;
      if (i >= J.n) break;
      for (long long e = i; e < i + 4 && e < J.n; ++e) {   // (the compiler vectorises the aligned case)
        float g = J.g[e];
        if constexpr (kScale) g *= gscale;
        const float d = g + wd * J.p[e];
        const float m = beta1 * J.m[e] + (1.f - beta1) * d;
        const float v = beta2 * J.v[e] + (1.f - beta2) * d * d;
        J.m[e] = m;
        J.v[e] = v;
        J.p[e] -= step * m / (sqrtf(v) / bc2_sqrt + eps);
      }
    }
  }
}

__global__ __launch_bounds__(256) void optimizer_step_kernel(const cavp_opt_job* __restrict__ jobs, int njobs, float lr_sgd,
                                                             float lr_adam, float momentum, float beta1, float beta2,
                                                             float eps, float bc1, float bc2_sqrt, int first_step) {
  optimizer_step_body<false>(jobs, njobs, lr_sgd, lr_adam, momentum, beta1, beta2, eps, bc1, bc2_sqrt, first_step);
}

// the same update with the per-step scalars of the state block (written by optimizer_schedule_kernel, the launch before this
// one on the stream; read-only here, so no workgroup depends on another)
__global__ __launch_bounds__(256) void optimizer_step_dev_kernel(const cavp_opt_job* __restrict__ jobs, int njobs, float momentum,
                                                                 float eps, const cavp_opt_state* __restrict__ state) {
  optimizer_step_body<false>(jobs, njobs, state->lr_sgd, state->lr_adam, momentum, state->beta1, state->beta2, eps, state->bc1,
                      state->bc2_sqrt, state->first_step);
}

// The scalars of step t in double precision, as the host computes them (optim.warmup_poly_lr, cavp_optimizer_step), rounded to f32
// once.  The reference sets the learning rate AFTER the optimiser step (trainer lr_step), so step t runs with get_lr(t - 1) and
// step 0 with the configured rate.  The plain and the guarded schedule kernel share it, so equal states give equal bits.
__device__ __forceinline__ float schedule_lr(const cavp_opt_state* state, long long t) {
  const double start = state->start_lr, end = state->end_lr;
  double lr = start;
  if (t > 0) {
    const long long cur = t - 1;
    if (cur < state->warmup_steps) {
      lr = start * ((double)cur / (double)state->warmup_steps);
    } else if (cur >= state->total_iters) {
      lr = end;   // outside the reference's domain (negative base of the power): defined as the end rate
    } else {
      lr = start * pow(1.0 - (double)cur / (double)state->total_iters, state->lr_power);
      lr = fmin(fmax(lr, end), start);
    }
  }
  return (float)lr;
}

// step t's scalars into the state block; then t + 1
__device__ __forceinline__ void schedule_advance(cavp_opt_state* state) {
  const long long t = state->t;
  const double n = (double)(t + 1);
  state->lr_sgd = schedule_lr(state, t);
  state->lr_adam = state->base_lr;
  state->bc1 = (float)(1.0 - pow((double)state->beta1, n));
  state->bc2_sqrt = (float)sqrt(1.0 - pow((double)state->beta2, n));
  state->first_step = t == 0;
  state->t = t + 1;
}

__global__ void optimizer_schedule_kernel(cavp_opt_state* state) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  schedule_advance(state);
}

// ---- step guard ---------------------------------------------------------------------------------------------------------------
// Four launches ordered by the stream: partials (one workgroup per optimiser block) -> finish (one workgroup) -> guarded
// schedule (one thread) -> guarded update.  No workgroup waits for another and nothing is accumulated with atomics.

__device__ __forceinline__ int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// sum of squares and non-finite count of one float4: a two-level tree
__device__ __forceinline__ void guard_acc4(const float4& g, float& ss, int& nf) {
  ss = (g.x * g.x + g.y * g.y) + (g.z * g.z + g.w * g.w);
  nf = nonfinite(g.x) + nonfinite(g.y) + nonfinite(g.z) + nonfinite(g.w);
}

// The update's block -> job mapping and element -> thread mapping; the gradients of the block are read once.  f32 tree: 2 levels
// inside a float4, 2 over a thread's four float4, 6 over the wave, 2 over the four waves = 12 levels, no chain.
__device__ __forceinline__ void grad_guard_partials_body(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                         cavp_guard_partial* __restrict__ partials) {
  __shared__ float s_ss[4];
  __shared__ int s_nf[4];
  const cavp_opt_job J = jobs[job_of_block(jobs, njobs)];
  const long long base = (long long)(blockIdx.x - J.blk0) * kElemsPerBlock;
  float ss[4] = {0.f, 0.f, 0.f, 0.f};
  int nf[4] = {0, 0, 0, 0};
  if (J.vec && base + kElemsPerBlock <= J.n) {   // a full block: the four 16-byte loads are in flight together
    float4 g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = *(const float4*)(J.g + base + (q * 256 + threadIdx.x) * 4ll);
#pragma unroll
    for (int q = 0; q < 4; ++q) guard_acc4(g[q], ss[q], nf[q]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long i = base + (q * 256 + threadIdx.x) * 4ll;
      if (i >= J.n) break;
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i + 4 <= J.n && J.vec) {
        g = *(const float4*)(J.g + i);
      } else {   // tails and unaligned views: scalar loads, zeros past the end
        g.x = J.g[i];
        if (i + 1 < J.n) g.y = J.g[i + 1];
        if (i + 2 < J.n) g.z = J.g[i + 2];
        if (i + 3 < J.n) g.w = J.g[i + 3];
      }
      guard_acc4(g, ss[q], nf[q]);
    }
  }
  float s = (ss[0] + ss[1]) + (ss[2] + ss[3]);
  int c = (nf[0] + nf[1]) + (nf[2] + nf[3]);
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_ss[wave] = s;
    s_nf[wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cavp_guard_partial out;
    out.sumsq = (s_ss[0] + s_ss[1]) + (s_ss[2] + s_ss[3]);
    out.nonfinite = (s_nf[0] + s_nf[1]) + (s_nf[2] + s_nf[3]);
    partials[blockIdx.x] = out;
  }
}

__global__ __launch_bounds__(256) void grad_guard_partials_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                  cavp_guard_partial* __restrict__ partials) {
  grad_guard_partials_body(jobs, njobs, partials);
}

constexpr int kFinishThreads = 1024, kFinishWaves = kFinishThreads / 64;

// One workgroup of 16 waves.  Wave w takes the jobs w, w + 16, ...; lane l adds that job's partials l, l + 64, ... in double, a
// butterfly adds the 64 lanes, the wave adds its jobs in ascending order, thread 0 adds the waves in ascending order: the order
// is a function of the job table alone.
__device__ __forceinline__ void grad_guard_finish_body(const cavp_opt_job* __restrict__ jobs, int njobs, int total_blocks,
                                                       const cavp_guard_partial* __restrict__ partials,
                                                       cavp_guard_state* __restrict__ guard) {
  __shared__ double s_ss[2][kFinishWaves];
  __shared__ long long s_nf[kFinishWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc_sgd = 0.0, acc_adam = 0.0;
  long long nf = 0;
  for (int j = wave; j < njobs; j += kFinishWaves) {
    const long long n = jobs[j].n;
    const int blk0 = jobs[j].blk0, kind = jobs[j].kind;
    int nblk = (int)((n + kElemsPerBlock - 1) / kElemsPerBlock);
    if (blk0 < 0 || blk0 > total_blocks) nblk = 0;
    if (nblk > total_blocks - blk0) nblk = total_blocks - blk0;   // never past the partials the launch before this one wrote
    double ss = 0.0;
    long long c = 0;
    for (int b = lane; b < nblk; b += 64) {
      const cavp_guard_partial P = partials[blk0 + b];
      ss += (double)P.sumsq;
      c += P.nonfinite;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ss += __shfl_xor(ss, o, 64);
      c += __shfl_xor(c, o, 64);
    }
    acc_sgd += kind == 0 ? ss : 0.0;
    acc_adam += kind == 0 ? 0.0 : ss;
    nf += c;
  }
  if (lane == 0) {
    s_ss[0][wave] = acc_sgd;
    s_ss[1][wave] = acc_adam;
    s_nf[wave] = nf;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sgd = 0.0, adam = 0.0;
  long long total_nf = 0;
  for (int w = 0; w < kFinishWaves; ++w) {
    sgd += s_ss[0][w];
    adam += s_ss[1][w];
    total_nf += s_nf[w];
  }
  // the coefficient comes from the norm in double and is rounded once (torch divides by its f32 norm: two roundings)
  const double norm_d = sqrt(sgd + adam);
  const float norm = (float)norm_d;
  const float max_norm = guard->max_norm;
  float coef = 1.f;
  if (max_norm > 0.f) coef = (float)fmin(1.0, (double)max_norm / (norm_d + 1e-6));
  guard->grad_norm = norm;
  guard->norm_sgd = (float)sqrt(sgd);
  guard->norm_adam = (float)sqrt(adam);
  guard->nonfinite = total_nf;
  guard->clip_coef = coef;
  guard->skip = (guard->skip_nonfinite & CAVP_GUARD_SKIP_GRADIENTS) != 0 && (total_nf > 0 || !isfinite(norm));
}

__global__ __launch_bounds__(kFinishThreads) void grad_guard_finish_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                           int total_blocks,
                                                                           const cavp_guard_partial* __restrict__ partials,
                                                                           cavp_guard_state* __restrict__ guard) {
  grad_guard_finish_body(jobs, njobs, total_blocks, partials, guard);
}

// One thread, behind the finish launch on the stream.
__device__ __forceinline__ void schedule_guarded_body(cavp_opt_state* state, cavp_guard_state* guard, const float* loss0,
                                                      const float* loss1) {
  const float l0 = loss0 ? loss0[0] : 0.f, l1 = loss1 ? loss1[0] : 0.f;
  int skip = guard->skip;
  // CAVP_GUARD_SKIP_LOSSES (a switch of its own): a loss that is not finite skips too.  The CE head turns "every label ignored"
  // into a NaN loss with ZERO gradients (train_pointwise.hip, inv = 0), which the gradients alone cannot show, and momentum +
  // weight decay would still move the weights.  The losses are the caller's: they must be the same on every rank.
  const int on_loss = (guard->skip_nonfinite & CAVP_GUARD_SKIP_LOSSES) != 0 && (nonfinite(l0) || nonfinite(l1));
  if (on_loss) {
    skip = 1;
    guard->skip = 1;   // the update launch behind this one reads it
  }
  cavp_step_record r;
  r.t = state->t;   // the index this step runs as (or would have run as)
  if (skip) {
    r.lr_sgd = schedule_lr(state, state->t);
    guard->skipped_total += 1;
  } else {
    schedule_advance(state);
    r.lr_sgd = state->lr_sgd;
  }
  r.nonfinite = guard->nonfinite;
  r.l_ce = l0;
  r.l_ctr = l1;
  r.grad_norm = guard->grad_norm;
  r.clip_coef = guard->clip_coef;
  r.flags = (skip ? CAVP_STEP_SKIPPED : 0) | (guard->clip_coef < 1.f ? CAVP_STEP_CLIPPED : 0) |
            (loss0 ? 0 : CAVP_STEP_NO_LOSS) | (loss1 ? 0 : CAVP_STEP_NO_LOSS1) | (on_loss ? CAVP_STEP_SKIPPED_LOSS : 0);
  const long long head = guard->head;
  const int history = guard->history > 0 ? guard->history : 1;
  cavp_step_record* ring = (cavp_step_record*)(guard + 1);
  ring[head % history] = r;
  guard->head = head + 1;
}

__global__ void optimizer_schedule_guarded_kernel(cavp_opt_state* state, cavp_guard_state* guard, const float* loss0,
                                                  const float* loss1) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  schedule_guarded_body(state, guard, loss0, loss1);
}

// the update with clip_coef * g; a skipped step returns before it touches a parameter or a state buffer
__global__ __launch_bounds__(256) void optimizer_step_guarded_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                     float momentum, float eps,
                                                                     const cavp_opt_state* __restrict__ state,
                                                                     const cavp_guard_state* __restrict__ guard) {
  if (guard->skip) return;
  optimizer_step_body<true>(jobs, njobs, state->lr_sgd, state->lr_adam, momentum, state->beta1, state->beta2, eps, state->bc1,
                            state->bc2_sqrt, state->first_step, guard->clip_coef);
}

// ---- gated twins (gradient accumulation, grad_accum.hip) -------------------------------------------------------------------------
// The six device-schedule kernels once more, each behind one word: *gate == 0 (a micro-step that does not close its window) and
// every workgroup returns before it reads or writes anything else; otherwise the SAME device bodies run, so a closing micro-step
// gives the bits of the ungated launch on an equal state.  The word is written by the accumulator's advance launch, earlier on
// the stream, and is read-only here: uniform over the launch, no workgroup depends on another.

__global__ void optimizer_schedule_gated_kernel(cavp_opt_state* state, const int32_t* __restrict__ gate) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || *gate == 0) return;
  schedule_advance(state);
}

__global__ __launch_bounds__(256) void optimizer_step_dev_gated_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                       float momentum, float eps,
                                                                       const cavp_opt_state* __restrict__ state,
                                                                       const int32_t* __restrict__ gate) {
  if (*gate == 0) return;
  optimizer_step_body<false>(jobs, njobs, state->lr_sgd, state->lr_adam, momentum, state->beta1, state->beta2, eps, state->bc1,
                             state->bc2_sqrt, state->first_step);
}

__global__ __launch_bounds__(256) void grad_guard_partials_gated_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                        cavp_guard_partial* __restrict__ partials,
                                                                        const int32_t* __restrict__ gate) {
  if (*gate == 0) return;
  grad_guard_partials_body(jobs, njobs, partials);
}

__global__ __launch_bounds__(kFinishThreads) void grad_guard_finish_gated_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                                 int total_blocks,
                                                                                 const cavp_guard_partial* __restrict__ partials,
                                                                                 cavp_guard_state* __restrict__ guard,
                                                                                 const int32_t* __restrict__ gate) {
  if (*gate == 0) return;
  grad_guard_finish_body(jobs, njobs, total_blocks, partials, guard);
}

__global__ void optimizer_schedule_guarded_gated_kernel(cavp_opt_state* state, cavp_guard_state* guard, const float* loss0,
                                                        const float* loss1, const int32_t* __restrict__ gate) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || *gate == 0) return;
  schedule_guarded_body(state, guard, loss0, loss1);
}

__global__ __launch_bounds__(256) void optimizer_step_guarded_gated_kernel(const cavp_opt_job* __restrict__ jobs, int njobs,
                                                                           float momentum, float eps,
                                                                           const cavp_opt_state* __restrict__ state,
                                                                           const cavp_guard_state* __restrict__ guard,
                                                                           const int32_t* __restrict__ gate) {
  if (*gate == 0 || guard->skip) return;
  optimizer_step_body<true>(jobs, njobs, state->lr_sgd, state->lr_adam, momentum, state->beta1, state->beta2, eps, state->bc1,
                            state->bc2_sqrt, state->first_step, guard->clip_coef);
}

}  // namespace

extern "C" int32_t cavp_optimizer_blocks(int64_t n) { return (int32_t)((n + kElemsPerBlock - 1) / kElemsPerBlock); }

extern "C" int cavp_optimizer_step(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float lr_sgd,
                                   float lr_adam, float momentum, float beta1, float beta2, float eps, int64_t step,
                                   void* stream) {
  if (!jobs_device || njobs <= 0 || total_blocks <= 0 || step < 1) return CAVP_ERR_BAD_ARG;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  optimizer_step_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, lr_sgd, lr_adam, momentum, beta1,
                                                                      beta2, eps, (float)bc1, (float)sqrt(bc2), step == 1);
  CHECK_LAUNCH();
}

extern "C" int64_t cavp_optimizer_state_bytes(void) { return (int64_t)sizeof(cavp_opt_state); }

extern "C" int cavp_optimizer_schedule(cavp_opt_state* state_device, void* stream) {
  if (!state_device) return CAVP_ERR_BAD_ARG;
  optimizer_schedule_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_optimizer_step_dev(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum,
                                       float eps, const cavp_opt_state* state_device, void* stream) {
  if (!jobs_device || !state_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  optimizer_step_dev_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, momentum, eps, state_device);
  CHECK_LAUNCH();
}

extern "C" int64_t cavp_guard_state_bytes(void) { return (int64_t)sizeof(cavp_guard_state); }
extern "C" int64_t cavp_step_record_bytes(void) { return (int64_t)sizeof(cavp_step_record); }

extern "C" int cavp_grad_guard_partials(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                        cavp_guard_partial* partials, void* stream) {
  if (!jobs_device || !partials || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  grad_guard_partials_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, partials);
  CHECK_LAUNCH();
}

extern "C" int cavp_grad_guard_finish(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                      const cavp_guard_partial* partials, cavp_guard_state* guard_device, void* stream) {
  if (!jobs_device || !partials || !guard_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  grad_guard_finish_kernel<<<1, kFinishThreads, 0, (hipStream_t)stream>>>(jobs_device, njobs, total_blocks, partials,
                                                                           guard_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_optimizer_schedule_guarded(cavp_opt_state* state_device, cavp_guard_state* guard_device, const float* loss0,
                                               const float* loss1, void* stream) {
  if (!state_device || !guard_device) return CAVP_ERR_BAD_ARG;
  optimizer_schedule_guarded_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state_device, guard_device, loss0, loss1);
  CHECK_LAUNCH();
}

extern "C" int cavp_optimizer_step_guarded(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum,
                                           float eps, const cavp_opt_state* state_device, const cavp_guard_state* guard_device,
                                           void* stream) {
  if (!jobs_device || !state_device || !guard_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  optimizer_step_guarded_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, momentum, eps, state_device,
                                                                               guard_device);
  CHECK_LAUNCH();
}

// ---- gated entry points: the launches above with the accumulator's gate word (cavp_accum_state.gate) ---------------------------
extern "C" int cavp_optimizer_schedule_gated(cavp_opt_state* state_device, const int32_t* gate_device, void* stream) {
  if (!state_device || !gate_device) return CAVP_ERR_BAD_ARG;
  optimizer_schedule_gated_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state_device, gate_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_optimizer_step_dev_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum,
                                             float eps, const cavp_opt_state* state_device, const int32_t* gate_device,
                                             void* stream) {
  if (!jobs_device || !state_device || !gate_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  optimizer_step_dev_gated_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, momentum, eps, state_device,
                                                                                 gate_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_grad_guard_partials_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                              cavp_guard_partial* partials, const int32_t* gate_device, void* stream) {
  if (!jobs_device || !partials || !gate_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  grad_guard_partials_gated_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, partials, gate_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_grad_guard_finish_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                            const cavp_guard_partial* partials, cavp_guard_state* guard_device,
                                            const int32_t* gate_device, void* stream) {
  if (!jobs_device || !partials || !guard_device || !gate_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  grad_guard_finish_gated_kernel<<<1, kFinishThreads, 0, (hipStream_t)stream>>>(jobs_device, njobs, total_blocks, partials,
                                                                                 guard_device, gate_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_optimizer_schedule_guarded_gated(cavp_opt_state* state_device, cavp_guard_state* guard_device,
                                                     const float* loss0, const float* loss1, const int32_t* gate_device,
                                                     void* stream) {
  if (!state_device || !guard_device || !gate_device) return CAVP_ERR_BAD_ARG;
  optimizer_schedule_guarded_gated_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state_device, guard_device, loss0, loss1, gate_device);
  CHECK_LAUNCH();
}

extern "C" int cavp_optimizer_step_guarded_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                                 float momentum, float eps, const cavp_opt_state* state_device,
                                                 const cavp_guard_state* guard_device, const int32_t* gate_device, void* stream) {
  if (!jobs_device || !state_device || !guard_device || !gate_device || njobs <= 0 || total_blocks <= 0) return CAVP_ERR_BAD_ARG;
  optimizer_step_guarded_gated_kernel<<<total_blocks, 256, 0, (hipStream_t)stream>>>(jobs_device, njobs, momentum, eps,
                                                                                     state_device, guard_device, gate_device);
  CHECK_LAUNCH();
}
