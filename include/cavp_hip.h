/*
 * cavp_hip.h — C-ABI of libcavp_hip.so: the MI355X (gfx950) kernels behind the CAVP forward hot path.
 *
 * The reference (cyh-0/CAVP) has no FFI / plugin layer: its "operators" are stock torch.nn modules called from
 * models/cavp_model.py::CAVP.forward.  Each entry point below therefore names the reference call site(s) whose
 * arithmetic it replaces (file:line relative to the reference repo).  The Python host in cavp_amd/ binds these
 * with ctypes and keeps the reference's nn.Module contract; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain pointers + sizes; no torch / C++ types.  All pointers are DEVICE pointers unless stated.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are launched asynchronously;
 *     nothing here allocates, frees or synchronises, so every call is hipGraph-capturable.
 *   - activations are NHWC ("channels-last"): element (n,h,w,c) of a tensor with pixel stride `ld` lives at
 *     ((n*H + h)*W + w)*ld + c.  `ld >= C` lets a kernel read/write a channel slice of a wider tensor
 *     (that is how torch.cat along C is done without a copy: encoder_decoder.py:104,139).
 *   - conv / linear weights are "OHWI": [Cout][KH][KW][Cin], i.e. the GEMM K dimension is contiguous.
 *   - dtype: CAVP_F32 (parity path, exact-f32 MFMA) or CAVP_BF16 (bf16 storage, f32 accumulate).
 *   - return value: 0 on success, negative cavp_status_t otherwise (see cavp_error_string).
 */
#ifndef CAVP_HIP_H_
#define CAVP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAVP_ABI_VERSION 16

typedef enum { CAVP_F32 = 0, CAVP_BF16 = 1, CAVP_I64 = 2 /* ABI 13: metrics inputs only */ } cavp_dtype_t;
typedef enum { CAVP_ACT_NONE = 0, CAVP_ACT_RELU = 1, CAVP_ACT_LEAKY = 2, CAVP_ACT_GELU = 3 } cavp_act_t;
typedef enum {
  CAVP_OK = 0,
  CAVP_ERR_BAD_ARG = -1,      /* null pointer / non-positive size */
  CAVP_ERR_UNSUPPORTED = -2,  /* shape the kernels do not cover (e.g. Cin not a multiple of the 16-byte vector) */
  CAVP_ERR_ALIGN = -3,        /* pointer or leading dimension not 16-byte aligned where required */
  CAVP_ERR_WORKSPACE = -4,    /* workspace too small */
  CAVP_ERR_LAUNCH = -5        /* hipLaunch failed (hipGetLastError != hipSuccess) */
} cavp_status_t;

int cavp_abi_version(void);

/* Clear nranges [start, end) element ranges (table_dev: int64 pairs in device memory; 4-float aligned) of one f32 buffer in one
 * launch: the per-step reset of the flat gradient arena.  max_len = the longest range (sizes the grid). */
int cavp_zero_ranges_f32(float* base, const int64_t* table_dev, int32_t nranges, int64_t max_len, void* stream);
/* ABI 11: clear nbytes (a multiple of 4, 4-byte aligned) of device memory: the training step's scratch pools and zero-initialised
 * gradients without a framework fill kernel on the path. */
int cavp_zero_bytes(void* p, size_t nbytes, void* stream);
/* ABI 11: *(int64_t*)table_dev[i] += inc for the n device addresses in table_dev (device memory): nn.BatchNorm2d's
 * num_batches_tracked counters of all layers (resnet.py:75-98 in train mode) in one launch. */
int cavp_i64_add_table(const int64_t* table_dev, int32_t n, int64_t inc, void* stream);
/* Opt-in deterministic training (the reference runs with cudnn.deterministic = True, main_vpo_mono.py:39-41).  With a scratch
 * buffer registered (>= 1 MiB, 16-byte aligned device memory that stays alive; 8 MiB covers every CAVP shape) the reductions
 * that otherwise finish with f32 atomics - cavp_colsum / cavp_colstats / cavp_bn_act_bwd_reduce, the dgamma / dbeta of
 * cavp_layernorm_bwd and the dk / dv of cavp_attn_gate_bwd - write per-workgroup partials and add them in a fixed order:
 * a training step is then bit-reproducible run to run.  scratch = NULL switches the mode off.  Process-wide (one process per
 * GPU); launches that need more scratch than registered return CAVP_ERR_WORKSPACE. */
int cavp_set_deterministic(void* scratch, size_t bytes);
int cavp_get_deterministic(void);
const char* cavp_error_string(int status);

/* ---------------------------------------------------------------------------------------------------------
 * Fused conv / linear: y = act( (conv(x, w) + nbias[n, :]) * scale + shift + residual )
 *
 * Replaces every nn.Conv2d(+BatchNorm2d eval)(+ReLU/LeakyReLU)(+residual add) group and every nn.Linear(+GELU /
 * ReLU) on the path:  resnet.py:75-98,107-121,186-190 (bottlenecks, stem convs 2-3) · encoder_decoder.py:62-75
 * (decoder head), :97-105 (reduce), :137-156 (ASPP) · vgg.py:17-36 (audio convs + FCs) · cavp_model.py:123-128,146
 * (projector Mlp) · attn.py:30-39,64-71,103-105,136-143 (patch_embed, q/k/v/proj, Mlp).
 *   scale/shift : per-Cout f32 (folded BN: scale = gamma/sqrt(var+eps), shift = beta - mean*scale; or bias).
 *                 scale == NULL means 1, shift == NULL means 0.
 *   nbias       : optional f32 [N][Cout], added per image before scale (ASPP pooled branch, :150-153).
 *   residual    : optional, same dtype as y, pixel stride ldr (Bottleneck `out += residual`, resnet.py:92-96;
 *                 attention residuals attn.py:148-149).
 *   A linear layer over T tokens is the 1x1 case with N=1, H=1, W=T.
 * Implicit GEMM on MFMA; taps that can never be in-bounds (dilation > extent) are skipped.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct cavp_conv_desc {
  int32_t dtype;      /* cavp_dtype_t of x, w, residual and y */
  int32_t N, H, W;    /* input batch / height / width */
  int32_t Cin, ldx;   /* input channels, input pixel stride (elements) */
  int32_t Cout, ldy;  /* output channels, output pixel stride */
  int32_t KH, KW, stride, pad, dil;
  int32_t ldr;        /* residual pixel stride (ignored when residual == NULL) */
  int32_t act;        /* cavp_act_t */
  int32_t splitk;     /* 0 = let the library choose; >= 1 forces that many K slices */
  int32_t tile;       /* 0 = auto; otherwise id (1..9) + profiling digits (tools/bench_conv.py): testing / tuning only */
  int32_t up;         /* 0/1 = ordinary conv.  up = s > 1 (power of two): x is read as if zero-upsampled by s, i.e. the
                         data-gradient of a stride-s conv (transposed conv); Ho/Wo below then give the output size */
  int32_t Ho, Wo;     /* only read when up > 1 (the forward conv's input extent) */
  int32_t stride_w;   /* 0 = same as `stride`; otherwise the horizontal stride (PVT spatial-reduction convs are run as
                         KH = sr, KW = 1 convs over the input viewed as [N][H][W/sr][sr*C] with stride (sr, 1)) */
  int32_t dw_oihw;    /* cavp_conv2d_wgrad_nhwc only: 1 = accumulate into a torch-layout [Cout][Cin][KH][KW] gradient (default 0: OHWI) */
  int32_t dw_overwrite; /* cavp_conv2d_wgrad_nhwc only: 1 = dw = gradient (beta = 0: dw is neither read nor required to be zeroed;
                           dead taps of a dilated kernel are written as zeros); default 0: dw += gradient */
  /* ---- ABI 6: epilogue fusions of the token path (cavp_conv2d_nhwc_aux) ---- */
  int32_t res_rows;   /* 0 = the residual has one row per output pixel; > 0: it has res_rows pixel rows and output pixel p
                         adds row p mod res_rows - the un-duplicated half of forward_train's `torch.cat((x, x.clone()))`
                         (cavp_model.py:181) read twice instead of copied (must be a multiple of 256 rows) */
  int32_t aux_mode;   /* 0 = none.  1 (act must be CAVP_ACT_GELU): besides y = gelu(t) the epilogue stores gelu'(t) into
                         `aux` (y's shape, stride ld_aux) - what the backward of timm's Mlp needs (attn.py:136-150,
                         cavp_model.py:123-128), so the pre-activation is never written.  2: the result is multiplied
                         element-wise by `aux` before the residual is added: d(pre) = d(hidden) * gelu'(pre) fused into
                         the data-gradient GEMM that produces d(hidden) */
  int32_t ld_aux;     /* pixel stride of aux (elements) */
} cavp_conv_desc;

size_t cavp_conv2d_workspace_bytes(const cavp_conv_desc* d);
/* tile_stats (optional, training): f32 [tiles][Cout][2]; the epilogue stores each pixel tile's per-channel mean and
 * centred second moment of the raw conv output, so BatchNorm batch statistics cost no extra pass (combine with
 * cavp_bn_finalize_tiles).  Only for plain convs (no scale/shift/nbias/residual/act) whose launch uses the staged
 * epilogue: query cavp_conv2d_tile_stats_layout first (returns 0 -> fall back to cavp_colsum + cavp_colstats). */
int cavp_conv2d_tile_stats_layout(const cavp_conv_desc* d, int32_t* tiles, int32_t* rows_per_tile);
int cavp_conv2d_nhwc(const cavp_conv_desc* d, const void* x, const void* w, const float* scale, const float* shift,
                     const float* nbias, const void* residual, void* y, void* workspace, size_t workspace_bytes,
                     float* tile_stats, void* stream);
/* The same with the auxiliary epilogue tensor of d->aux_mode (dtype of y; written for mode 1, read for mode 2).  Launches
 * that use res_rows / aux_mode need the 16-byte epilogue (Cout, ldy, ldr, ld_aux multiples of 8 bf16 / 4 f32 elements,
 * 16-byte aligned pointers) and are never split over K: CAVP_ERR_UNSUPPORTED otherwise. */
int cavp_conv2d_nhwc_aux(const cavp_conv_desc* d, const void* x, const void* w, const float* scale, const float* shift,
                         const float* nbias, const void* residual, void* y, void* aux, void* workspace,
                         size_t workspace_bytes, float* tile_stats, void* stream);
/* ABI 10: BatchNorm-backward statistics fused into the data-gradient launch that PRODUCES the gradient of a BatchNorm + activation
 * output.  torch.autograd runs ReLU.backward and BatchNorm.backward as passes of their own behind every conv's backward
 * (resnet.py:75-98 under trainer_cavp_vpo_mono.py:190 `loss.backward()`); here the conv launch (a data gradient: d = the
 * transposed conv, see `up`) finishes v = conv(x, w) + residual, multiplies by the activation's derivative, stores
 *   g = v * act'(.)                      (act' from `out`, the forward's activation output, or re-derived from z*fwd_scale + fwd_shift)
 * and writes, per pixel tile, partials[tile][c] = (sum g, sum g * (z - mean) * rstd) over the tile's rows - the two reductions of
 * cavp_bn_act_bwd_reduce, which then only have to be summed over the tiles (cavp_bn_bwd_sum_tiles; fixed order, no atomics).
 * cavp_bn_act_bwd_apply runs on g with act = NONE.  cavp_conv2d_bnbwd_layout returns 0 when the launch cannot carry the
 * statistics (split over K, 256 x 256 tile, unaligned operands): the caller keeps the separate reduce. */
typedef struct cavp_bnbwd_args {
  const void* z;            /* the BatchNorm's input (dtype and shape of y), pixel stride ld_z */
  const void* out;          /* the activation's output (BN + residual + act), pixel stride ld_out; NULL: mask from z, fwd_scale, fwd_shift */
  int32_t ld_z, ld_out;
  const float* fwd_scale;   /* the forward's folded scale / shift (only read when out == NULL and act != NONE) */
  const float* fwd_shift;
  const float* mean;        /* batch mean and 1 / sqrt(var + eps) of z */
  const float* rstd;
  int32_t act;              /* CAVP_ACT_NONE / RELU / LEAKY */
  int32_t pad_;
  float* partials;          /* f32 [tiles][Cout][2] (cavp_conv2d_bnbwd_layout): per pixel tile (sum g, sum g * zhat), summed by cavp_bn_bwd_sum_tiles */
} cavp_bnbwd_args;   /* (ABI 11: the f32-atomic route of ABI 10 - sum_g / sum_gz - is gone: measured slower, profiles/r05_notes.md 3) */
int cavp_conv2d_bnbwd_layout(const cavp_conv_desc* d, int32_t* tiles, int32_t* rows_per_tile);
int cavp_conv2d_nhwc_bnbwd(const cavp_conv_desc* d, const void* x, const void* w, const void* residual, void* y,
                           const cavp_bnbwd_args* b, void* workspace, size_t workspace_bytes, void* stream);
/* sum_g[c] += sum_t partials[t][c][0], sum_gz[c] += sum_t partials[t][c][1] (ascending tiles within 16 interleaved lanes, then a
 * fixed tree: deterministic). */
int cavp_bn_bwd_sum_tiles(const float* partials, int32_t tiles, int32_t C, float* sum_g, float* sum_gz, void* stream);
/* cavp_bn_act_bwd_apply (below) that also adds the two sums to the BatchNorm's affine gradients (dbeta_acc += sum_g, dgamma_acc +=
 * sum_gz; both or neither): for sums that arrive in scratch memory (the atomic route of cavp_conv2d_nhwc_bnbwd). */
int cavp_bn_act_bwd_apply_acc(int32_t dtype, const void* dy, const void* y, const void* z, const float* mean, const float* rstd,
                              const float* gamma, const float* sum_g, const float* sum_gz, int64_t rows, int32_t C, int32_t ld_dy,
                              int32_t ld_y, int32_t ld_z, int32_t act, void* dz, int32_t ld_dz, void* g_out, int32_t ld_g,
                              const float* fwd_scale, const float* fwd_shift, float* dbeta_acc, float* dgamma_acc, void* stream);
/* An automatically planned launch of the 256x256 tile whose last round of 256 tiles is at most a quarter full (the decoder head
 * convs, encoder_decoder.py:62-75, at 2B x 56 x 56: 784 tiles = 3.06 rounds) is issued as the leading images on the 256x256 tile
 * + the remaining images on the small tiles.  Process-wide switch for A/B runs and tests (default on); results are identical
 * either way up to the summation order inside the tail images. */
int cavp_set_tail_split(int32_t on);
/* ABI 9: the 256 x 256 weight-gradient tile (csrc/conv_wgrad_big.hip; bf16: one workgroup per CU, four-stage LDS-DMA
 * ring, v_mfma_f32_32x32x16_bf16) for the weight gradients of encoder_decoder.py:62-75 (decoder head), models/attn.py:136-143 and
 * cavp_model.py:123-128 (token / projector Mlp) - the jobs with >= 16384 pixel rows and >= 192 input and output channels.
 * mode: 0 (default) = those jobs, 1 = never (the 128 x 128 tile everywhere), 2 = every bf16 job (tests).  schedule: 2 (default) =
 * sixteen waves per workgroup (64 x 64 wave tiles, four waves per SIMD, fragments double-buffered by k step), 1 = eight waves
 * (64 x 128 wave tiles) with every LDS read and DMA issue in the gaps between the MFMAs, 0 = eight waves: read, multiply, retire,
 * fetch.  Same products, same summation order in all three.  The choice of tile depends on the job alone, so grouped and single
 * launches of a job with one split count stay bit-identical.  Process-wide switch for A/B runs and tests. */
int cavp_set_wgrad_big(int32_t mode, int32_t schedule);

/* Direct 3x3 conv for Cin in {1,2,3} reading an NCHW f32 tensor and writing NHWC (dtype) with scale/shift + act:
 * the ResNet deep-stem first conv (resnet.py:108-110, stride 2) and the first VGGish conv (vgg.py:26-36). */
int cavp_conv3x3_smallcin_nchw(int32_t dtype, const float* x_nchw, const float* w_oihw, const float* scale,
                               const float* shift, void* y_nhwc, int32_t N, int32_t Cin, int32_t H, int32_t W,
                               int32_t Cout, int32_t stride, int32_t act, void* stream);

/* nn.MaxPool2d(k, s, p) on NHWC (resnet.py:139,190: 3/2/1; vgg.py:30: 2/2/0).  argmax (optional, u8 [N][Ho][Wo][C]):
 * window-relative position kh*k + kw of the first maximum in scan order (the element ATen routes the gradient to),
 * consumed by cavp_maxpool_bwd_nhwc. */
int cavp_maxpool_nhwc(int32_t dtype, const void* x, void* y, uint8_t* argmax, int32_t N, int32_t H, int32_t W,
                      int32_t C, int32_t k, int32_t stride, int32_t pad, void* stream);

/* ABI 12.  The same pool over act(x * scale + shift) (per-channel f32 scale / shift, rounded to dtype before the comparison): the training step's
 * BatchNorm apply + ReLU in front of the stem pool (resnet.py:187-190: bn1 -> relu -> maxpool) without the activation tensor in memory.
 * Values and arg-max are bit-identical to cavp_scale_shift_act followed by cavp_maxpool_nhwc. */
int cavp_maxpool_affine_nhwc(int32_t dtype, const void* x, const float* scale, const float* shift, int32_t act, void* y,
                             uint8_t* argmax, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad,
                             void* stream);

/* x.view(N, C, -1).mean(-1) for NHWC x; output f32 [N][C] (ASPP._global_pooling, encoder_decoder.py:158-161). */
int cavp_global_avgpool_nhwc(int32_t dtype, const void* x, float* y, int32_t N, int32_t HW, int32_t C, int32_t ldx,
                             void* stream);

/* F.interpolate(mode="bilinear") NHWC -> NHWC channel slice (encoder_decoder.py:103, align_corners=True). */
int cavp_bilinear_nhwc(int32_t dtype, const void* x, void* y, int32_t N, int32_t Hi, int32_t Wi, int32_t C,
                       int32_t ldx, int32_t Ho, int32_t Wo, int32_t ldy, int32_t align_corners, void* stream);

/* Final F.interpolate(..., align_corners=False) of the logits: NHWC (dtype) in, NCHW f32 out (cavp_model.py:140). */
int cavp_bilinear_nhwc_to_nchw(int32_t dtype, const void* x, float* y_nchw, int32_t N, int32_t Hi, int32_t Wi,
                               int32_t C, int32_t ldx, int32_t Ho, int32_t Wo, int32_t align_corners, void* stream);

/* nn.LayerNorm(C, eps) over the last dim of [rows][C] (attn.py:130,136,229 -> :154-155,149,242). */
int cavp_layernorm(int32_t dtype, const void* x, const float* gamma, const float* beta, void* y, int32_t rows,
                   int32_t C, int32_t ldx, int32_t ldy, float eps, void* stream);
/* residual + DropPath + LayerNorm of a transformer block's stream in one pass (pvt.py:252-256 with timm's drop_path):
 * y_sum = x + row_scale[row / rows_per_group] * branch (dense [rows][C], x's dtype), y = LayerNorm(y_sum).  branch = NULL: plain
 * cavp_layernorm. */
int cavp_layernorm_residual(int32_t dtype, const void* x, const void* branch, const float* row_scale, int32_t rows_per_group,
                            const float* gamma, const float* beta, void* y_sum, void* y, int32_t rows, int32_t C, int32_t ldx,
                            int32_t ldy, float eps, void* stream);

/* Sigmoid-gated single-key attention (attn.py:73-106 with N_kv == 1):
 *   s[b,h,t] = sigmoid(scale * <q[b,t,h,:], k[b,h,:]>);  o[b,t,h,:] = s[b,h,t] * v[b,h,:];  attn[b,h,t] = s.
 * q: [q_batch][T][heads*hd], o: [B][T][heads*hd] (dtype); k,v: [B][heads*hd] (dtype); attn: f32 [B][heads][T].
 * q_batch = B, or a divisor of B: batch item b reads q[b mod q_batch] (forward_train runs the query projection once on the B
 * images and gates it with the 2B audio clips, cavp_model.py:181). */
int cavp_attn_gate(int32_t dtype, const void* q, const void* k, const void* v, void* o, float* attn, int32_t B,
                   int32_t T, int32_t heads, int32_t hd, float scale, int32_t q_batch, void* stream);

/* BatchNorm (eval) folding: scale = gamma * rsqrt(var + eps), shift = beta - mean * scale (f32, C entries). */
int cavp_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* scale,
                 float* shift, int32_t C, void* stream);

/* Weight packing: OIHW f32 (torch layout) -> OHWI (dtype).  Linear weights are the KH=KW=1 case (pure cast). */
int cavp_pack_weight_ohwi(int32_t dtype, const float* w_oihw, void* w_ohwi, int32_t Cout, int32_t Cin, int32_t KH,
                          int32_t KW, void* stream);

/* Element-wise cast between f32 and dtype (n elements): src_dtype -> dst_dtype. */
int cavp_cast(int32_t src_dtype, const void* src, int32_t dst_dtype, void* dst, int64_t n, void* stream);

/* =========================================================================================================
 * Training side: batch-statistics BatchNorm and the backward kernels.  The reference gets all
 * of this from torch.autograd over the modules cited above (trainer_cavp_vpo_mono.py:168-193 `loss.backward()`).
 * Data gradients of conv / linear reuse cavp_conv2d_nhwc with cavp_pack_weight_dgrad weights (+ `up` for strides).
 * ======================================================================================================= */

/* Weight gradient of a conv / linear: dw[co][kh][kw][ci] += sum_pixels dy[pix][co] * x[pix @ tap][ci] (f32, OHWI; the
 * result is ADDED to dw).  Fields of `d` describe the FORWARD conv (x is its input, dy its output gradient with pixel
 * stride d->ldy).  The pixel reduction is split over workgroups; partial slabs go to `workspace`
 * (cavp_conv2d_wgrad_workspace_bytes) and are reduced in a fixed order: deterministic, no atomics.
 * dbias (optional, f32 [Cout]): dbias[co] += sum_pixels dy[pix][co], the bias gradient, summed from the dY tiles the kernel
 * streams anyway (saves the separate column-sum pass over dY). */
size_t cavp_conv2d_wgrad_workspace_bytes(const cavp_conv_desc* d);
int cavp_conv2d_wgrad_nhwc(const cavp_conv_desc* d, const void* x, const void* dy, float* dw_ohwi, float* dbias,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ABI 7: up to CAVP_WGRAD_GROUP_MAX independent weight gradients (the jobs of cavp_conv2d_wgrad_nhwc, one dtype) in ONE launch
 * (+ one launch for the slab reduces of the jobs that split their pixel range).  torch.autograd computes every weight
 * gradient where its layer's backward runs (trainer_cavp_vpo_mono.py:168-193 `loss.backward()`); nothing in the backward
 * chain consumes them, so the host defers the weight gradients of a stage of small layers (ResNet layer3: 19 convs on
 * 32 x 14 x 14 pixels, resnet.py:75-98; the 52 PVTv2 blocks, pvt.py:137-170) and issues them together: the launches fill the
 * chip with far fewer pixel splits (less slab traffic, one reduce instead of 19).  `jobs` is a HOST array; the job table
 * travels as kernel arguments.  Two jobs must not share a dw or dbias (CAVP_ERR_BAD_ARG).  The split reduction stays a
 * fixed-order slab sum: deterministic. */
#define CAVP_WGRAD_GROUP_MAX 16
typedef struct cavp_wgrad_job {
  cavp_conv_desc desc;   /* the FORWARD conv, as for cavp_conv2d_wgrad_nhwc (dw_oihw / dw_overwrite / splitk honoured per job) */
  const void* x;
  const void* dy;
  float* dw;
  float* dbias;          /* optional */
} cavp_wgrad_job;
size_t cavp_conv2d_wgrad_group_workspace_bytes(const cavp_wgrad_job* jobs, int32_t njobs);
int cavp_conv2d_wgrad_group(const cavp_wgrad_job* jobs, int32_t njobs, void* workspace, size_t workspace_bytes, void* stream);

/* OIHW f32 -> [Cin][KH][KW][Cout] (dtype), taps rotated by 180 degrees: the OHWI weight of the transposed conv. */
/* All weight re-packs of one training step in one launch per <= 48 tensors (the per-tensor entry points cost ~170
 * launches of ~8 us each per step, profiles/r01_notes.md): for every job, w_oihw f32 [Cout][Cin][KH][KW] ->
 * ohwi (cavp_pack_weight_ohwi layout, may be NULL) and dgrad (cavp_pack_weight_dgrad layout, may be NULL), both `dtype`.
 * `jobs` is a HOST array; device pointers inside. */
typedef struct cavp_pack_job {
  const float* w_oihw;
  void* ohwi;
  void* dgrad;
  int32_t Cout, Cin, KH, KW;
} cavp_pack_job;
int cavp_pack_weights_multi(int32_t dtype, const cavp_pack_job* jobs, int32_t njobs, void* stream);
int cavp_pack_weight_dgrad(int32_t dtype, const float* w_oihw, void* w_t, int32_t Cout, int32_t Cin, int32_t KH,
                           int32_t KW, void* stream);
/* OHWI f32 gradient -> OIHW f32 (.grad layout); accumulate != 0 adds into the destination. */
int cavp_unpack_weight_grad(const float* g_ohwi, float* g_oihw, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                            int32_t accumulate, void* stream);
/* Weight gradient of cavp_conv3x3_smallcin_nchw: dw_oihw (f32) += im2col(x)^T dy on the MFMA weight-gradient kernel
 * (deterministic).  workspace: cavp_conv3x3_smallcin_wgrad_workspace_bytes(...) bytes, 16-byte aligned. */
size_t cavp_conv3x3_smallcin_wgrad_workspace_bytes(int32_t dtype, int32_t N, int32_t Cin, int32_t H, int32_t W,
                                                   int32_t Cout, int32_t stride);
int cavp_conv3x3_smallcin_wgrad(int32_t dtype, const float* x_nchw, const void* dy_nhwc, float* dw_oihw, int32_t N,
                                int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t stride, void* workspace,
                                size_t workspace_bytes, void* stream);

/* nn.BatchNorm2d in training mode (resnet.py / encoder_decoder.py BN layers under model.train()):
 *   cavp_colstats     sum[c] += sum_rows (x - s_c), sumsq[c] += sum_rows (x - s_c)^2 with an optional per-channel
 *                     shift s (f32 atomics; caller zeroes).  Two passes (s = 0, then s = mean) give a cancellation-free
 *                     variance, which matters for the tiny-M BatchNorms (ASPP pooled branch: M = batch size).
 *   cavp_bn_finalize  mean = s + sum/M, var = sumsq/M - (sum/M)^2 -> scale = gamma*rstd, shift = beta - mean*scale;
 *                     saves mean, rstd; updates the running
 *                     statistics in place (momentum, unbiased variance) when running_mean/var are non-NULL
 *   cavp_scale_shift_act  y = act(x*scale + shift + residual)
 *   cavp_bn_act_bwd_reduce / _apply  g = dy*act'(y); dbeta = sum g; dgamma = sum g*zhat;
 *                     dz = gamma*rstd*(g - dbeta/M - zhat*dgamma/M); optional g_out = g (skip-path gradient) */
int cavp_colstats(int32_t dtype, const void* x, const float* shift, int64_t rows, int32_t C, int32_t ldx, float* sum,
                  float* sumsq, void* stream);
int cavp_scale_f32(const float* in, float alpha, float* out, int32_t n, void* stream); /* out = alpha * in */
int cavp_bn_finalize(const float* sum, const float* sumsq, const float* stat_shift, int64_t count, const float* gamma,
                     const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                     float* mean, float* rstd, int32_t C, void* stream);
int cavp_bn_finalize_tiles(const float* tile_stats, int32_t tiles, int32_t rows_per_tile, int64_t count,
                           const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                           float* running_var, float* scale, float* shift, float* mean, float* rstd, int32_t C,
                           void* stream);
/* SyncBatchNorm (main_vpo_mono.py:130): this rank's per-channel (mean, M2) from its tile statistics, f32 [C][2].  The ranks'
 * moments are all-gathered into [world][C][2] and combined by cavp_bn_finalize_tiles(tiles = world, rows_per_tile = the
 * per-rank row count): ONE collective per BatchNorm layer in the forward. */
int cavp_bn_tiles_to_moments(const float* tile_stats, int32_t tiles, int32_t rows_per_tile, int64_t count, float* moments,
                             int32_t C, void* stream);
int cavp_scale_shift_act(int32_t dtype, const void* x, const float* scale, const float* shift, const void* residual,
                         void* y, int64_t rows, int32_t C, int32_t ldx, int32_t ldr, int32_t ldy, int32_t act,
                         void* stream);
/* y may be NULL for a BN + activation WITHOUT residual: the activation mask is then re-derived from z with the forward's
 * folded fwd_scale / fwd_shift (y = act(z*scale + shift) > 0 <=> z*scale + shift > 0), which saves reading y in both passes */
int cavp_bn_act_bwd_reduce(int32_t dtype, const void* dy, const void* y, const void* z, const float* mean,
                           const float* rstd, int64_t rows, int32_t C, int32_t ld_dy, int32_t ld_y, int32_t ld_z,
                           int32_t act, float* sum_g, float* sum_gz, const float* fwd_scale, const float* fwd_shift,
                           void* stream);
int cavp_bn_act_bwd_apply(int32_t dtype, const void* dy, const void* y, const void* z, const float* mean,
                          const float* rstd, const float* gamma, const float* sum_g, const float* sum_gz, int64_t rows,
                          int32_t C, int32_t ld_dy, int32_t ld_y, int32_t ld_z, int32_t act, void* dz, int32_t ld_dz,
                          void* g_out, int32_t ld_g, const float* fwd_scale, const float* fwd_shift, void* stream);
/* Tile combine inside the apply pass, for launches with few tiles (added to ABI 16).
 *   cavp_bn_tiles_scale_shift_act = cavp_bn_finalize_tiles(count = rows) + cavp_scale_shift_act in ONE launch: every workgroup
 *     combines the [tiles][C][2] (mean, M2) table for its own 64-channel slice; one workgroup per slice writes scale, shift,
 *     mean, rstd and updates the running statistics.
 *   cavp_bn_tiles_bwd_apply = cavp_bn_bwd_sum_tiles + cavp_bn_act_bwd_apply(y = NULL, act = CAVP_ACT_NONE, no g_out) in ONE launch:
 *     dz is computed from the partials alone and the sums are ADDED to sum_g / sum_gz, which must be zero on entry.
 * Both give bit-identical results to the two launches they replace.  CAVP_ERR_UNSUPPORTED (nothing launched: use the two
 * launches) when tiles exceeds the fused limit, when C or a leading dimension is not a multiple of the 16-byte vector, when a
 * tensor is not 16-byte aligned, or for an unhandled dtype. */
int cavp_bn_tiles_scale_shift_act(int32_t dtype, const void* x, const float* tile_stats, int32_t tiles, int32_t rows_per_tile,
                                  const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                  float* running_var, float* scale, float* shift, float* mean, float* rstd, const void* residual,
                                  void* y, int64_t rows, int32_t C, int32_t ldx, int32_t ldr, int32_t ldy, int32_t act, void* stream);
int cavp_bn_tiles_bwd_apply(int32_t dtype, const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                            const float* partials, int32_t tiles, float* sum_g, float* sum_gz, int64_t rows, int32_t C,
                            int32_t ld_dy, int32_t ld_z, void* dz, int32_t ld_dz, void* stream);
/* dx = dy * act'(.): ReLU / LeakyReLU from the activation OUTPUT, GELU from the pre-activation (ref). */
int cavp_act_bwd(int32_t dtype, const void* dy, const void* ref, void* dx, int64_t rows, int32_t C, int32_t ld_dy,
                 int32_t ld_ref, int32_t ld_dx, int32_t act, void* stream);
int cavp_add(int32_t dtype, const void* a, const void* b, void* out, int64_t n, void* stream);
/* out[c] += sum_rows x[r][c]  (bias gradients; f32 atomics, caller zeroes) */
int cavp_colsum(int32_t dtype, const void* x, int64_t rows, int32_t C, int32_t ldx, float* out, void* stream);
/* BatchNorm batch statistics of a tensor whose producer could not fuse them: per-tile (mean, M2) of 128-row tiles in one pass,
 * tile_stats f32 [ceil(rows / 128)][C][2] - the layout cavp_bn_finalize_tiles(tiles, rows_per_tile = 128) combines. */
int cavp_col_tile_stats(int32_t dtype, const void* x, int64_t rows, int32_t C, int32_t ldx, float* tile_stats, void* stream);
/* out[g][c] += sum of rows g*rows_per_group .. (g+1)*rows_per_group - 1: the per-image bias gradient of the ASPP pooled branch
 * (encoder_decoder.py:150-154) for all images in one launch.  Deterministic (one owner per output). */
int cavp_colsum_groups(int32_t dtype, const void* x, int32_t groups, int32_t rows_per_group, int32_t C, int32_t ldx, float* out,
                       void* stream);
/* nn.LayerNorm backward; dgamma / dbeta are accumulated with f32 atomics (caller zeroes). */
int cavp_layernorm_bwd(int32_t dtype, const void* dy, const void* x, const float* gamma, void* dx, float* dgamma,
                       float* dbeta, int32_t rows, int32_t C, int32_t ld_dy, int32_t ld_x, int32_t ld_dx, float eps,
                       void* stream);
/* same, with the gradient the input already holds added in: dx = layernorm_bwd(dy) + dx_add (dx_add may be NULL, and may be dx
 * itself).  The residual stream of a transformer block (pvt.py:252-256, attn.py:194-197) reaches the norm's input twice.
 * dx_scaled (optional, dense [rows][C]): a second copy of dx with row r multiplied by row_scale[r / rows_per_group] - the
 * gradient of a DropPath branch (timm drop_path: mask / keep per image) that hangs off the same residual stream. */
int cavp_layernorm_bwd_add(int32_t dtype, const void* dy, const void* x, const float* gamma, const void* dx_add, int32_t ld_add,
                           void* dx, void* dx_scaled, const float* row_scale, int32_t rows_per_group, float* dgamma,
                           float* dbeta, int32_t rows, int32_t C, int32_t ld_dy, int32_t ld_x, int32_t ld_dx, float eps,
                           void* stream);
/* ---- cross-modal attention with ONE key / value token per batch item, collapsed to rank-H operations (ABI 8) ------------------
 * attn.py:73-106 as CAVP calls it (x_k = x_v = the audio token, cavp_model.py:145-149; 4 heads, q / k / v without bias, sigmoid):
 *   q = x Wq^T, s[t,h] = scale q[t,h,:] . k[h,:], g = sigmoid(s), o[t,h,:] = g[t,h] v[h,:], out = x + o Wp^T + bp   (attn.py:153-156)
 * equals, with u[b,h,:] = scale Wq[h-slice,:]^T k[b,h-slice] and p[b,h,:] = Wp[:,h-slice] v[b,h-slice] (H x C per batch item),
 *   g[b,t,h] = sigmoid(x[t,:] . u[b,h,:]),   out[b,t,:] = x[t,:] + bp + sum_h g[b,t,h] p[b,h,:]
 * so the two C x C token GEMMs (and their data / weight gradient GEMMs) become one pass over the tokens per direction.
 * wq, wp: the f32 [C][C] weights of attn.q / attn.proj (nn.Linear layout); k, v: [B][C] in `dtype`; U, P: f32 [B][heads][C].
 * x: [xb][T][C] with xb dividing B (forward_train duplicates the images, cavp_model.py:181: batch item b reads x[b % xb]).
 * Supported: heads == 4, C <= 512, C % 8 == 0 (cavp_attn1_supported); callers keep cavp_attn_gate + two linears otherwise. */
int cavp_attn1_supported(int32_t C, int32_t heads);
int cavp_attn1_prepare(int32_t dtype, const float* wq, const float* wp, const void* k, const void* v, float* U, float* P, int32_t B,
                       int32_t C, int32_t heads, float scale, void* stream);
/* out: [B][T][C] in `dtype`; attn: f32 [B][heads][T] (the reference's attn_v, cavp_model.py:150); bp may be NULL. */
int cavp_attn1_fwd(int32_t dtype, const void* x, const float* U, const float* P, const float* bp, void* out, float* attn, int32_t B,
                   int32_t xb, int32_t T, int32_t C, int32_t heads, void* stream);
/* Backward over the tokens: dx [xb][T][C] = sum over the batch items that share a row of (dout + sum_h ds[t,h] u[b,h,:]) is
 * WRITTEN (not accumulated); dU / dP: f32 [B][heads][C] written; dbp (optional, f32 [C]) accumulated.  All sums in a fixed
 * order (per-workgroup slabs in `workspace`, cavp_attn1_bwd_workspace_bytes). */
size_t cavp_attn1_bwd_workspace_bytes(int32_t B, int32_t xb, int32_t T, int32_t C, int32_t heads);
int cavp_attn1_bwd(int32_t dtype, const void* dout, const void* x, const float* U, const float* P, void* dx, float* dU, float* dP,
                   float* dbp, void* workspace, size_t workspace_bytes, int32_t B, int32_t xb, int32_t T, int32_t C, int32_t heads,
                   void* stream);
/* dwq, dwp (f32 [C][C], nn.Linear layout) accumulated; dk, dv: f32 [B][C] written. */
int cavp_attn1_finish(int32_t dtype, const float* wq, const float* wp, const void* k, const void* v, const float* dU, const float* dP,
                      float* dwq, float* dwp, float* dk, float* dv, int32_t B, int32_t C, int32_t heads, float scale, void* stream);
/* backward of cavp_attn_gate; dk, dv: f32 [B][heads*hd] accumulated with atomics (caller zeroes); dattn optional.
 * q: [q_batch][T][heads*hd] as in the forward; dq: [B][T][heads*hd] (the caller sums the q_batch-periodic parts). */
int cavp_attn_gate_bwd(int32_t dtype, const void* dout, const void* q, const void* k, const void* v, const float* attn,
                       const float* dattn, void* dq, float* dk, float* dv, int32_t B, int32_t T, int32_t heads,
                       int32_t hd, float scale, int32_t q_batch, void* stream);
/* dx [N][H][W][C] = gradient routed to the recorded arg-max of every window (argmax from cavp_maxpool_nhwc) */
int cavp_maxpool_bwd_nhwc(int32_t dtype, const uint8_t* argmax, const void* dy, void* dx, int32_t N, int32_t H, int32_t W,
                          int32_t C, int32_t k, int32_t stride, int32_t pad, void* stream);
int cavp_bilinear_bwd_nhwc(int32_t dtype, const void* dy, void* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t C,
                           int32_t ld_dx, int32_t Ho, int32_t Wo, int32_t ld_dy, int32_t align_corners, void* stream);
/* backward of cavp_bilinear_nhwc_to_nchw: dy NCHW f32 (images >= n_valid carry zero gradient), dx NHWC (dtype) */
int cavp_bilinear_bwd_nchw_to_nhwc(int32_t dtype, const float* dy_nchw, void* dx, int32_t N, int32_t n_valid,
                                   int32_t Hi, int32_t Wi, int32_t C, int32_t ld_dx, int32_t Ho, int32_t Wo,
                                   int32_t align_corners, void* stream);
/* x[n, p, :] += alpha * v[n, :]  (global-average-pool backward) */
int cavp_bcast_add_nhwc(int32_t dtype, void* x, const float* v, float alpha, int32_t N, int32_t HW, int32_t C,
                        int32_t ld, void* stream);
/* nn.CrossEntropyLoss(ignore_index) on NCHW f32 logits of the first n_img images (loss/losser.py:60-62 applied to
 * `out[:B] + out[B:]*0`, trainer_cavp_vpo_mono.py:171,187): loss[0] = mean over valid pixels; dlogits (optional,
 * [n_total][C][HW]) = grad_scale * dloss/dlogits, zero for images >= n_img.  scratch: CAVP_CE_SCRATCH_FLOATS floats
 * (per-workgroup partial sums, combined in a fixed order: the loss is bit-reproducible run to run). */
#define CAVP_CE_SCRATCH_FLOATS (2 + 2 * 1024)
int cavp_ce_loss_nchw(const float* logits, const int64_t* labels, int32_t n_img, int32_t n_total, int32_t C, int64_t HW,
                      int32_t ignore_index, float grad_scale, float* loss, float* dlogits, float* scratch,
                      void* stream);
/* SURVEY.md §8f row f1 - the head of the training step in one op: F.interpolate(bilinear) of the low-resolution logits
 * (models/cavp_model.py:143-146) + CrossEntropyLoss(ignore_index) on `out[:n_img] + out[n_img:]*0`
 * (trainer_cavp_vpo_mono.py:171,187; loss/losser.py:60-62) + the gradient w.r.t. the low-resolution logits, without
 * the [n_total][C][Ho][Wo] f32 prediction or its gradient ever reaching HBM.
 *   lo, dlo: [n_total][Hi][Wi][ld] (dtype), classes in columns [0, C); dlo (optional) = grad_scale * dloss/dlo with every
 *            column written (padding columns and images >= n_img: zero)
 *   labels:  int64 [n_img][Ho][Wo];  lse: f32 [n_img][Ho][Wo] workspace (per-pixel log-sum-exp);
 *   scratch: CAVP_CE_SCRATCH_FLOATS floats;  loss[0] = mean over the valid pixels (fixed summation order). */
int cavp_upsample_ce_head(int32_t dtype, const void* lo, const int64_t* labels, int32_t n_img, int32_t n_total, int32_t C,
                          int32_t Hi, int32_t Wi, int32_t ld, int32_t Ho, int32_t Wo, int32_t align_corners,
                          int32_t ignore_index, float grad_scale, float* loss, void* dlo, float* lse, float* scratch,
                          void* stream);

/* ---- fused optimiser step (harness row of SURVEY.md §8c): torch.optim.SGD(momentum, weight_decay) on the visual groups +
 * torch.optim.Adam on the audio encoder (main_vpo_mono.py:45-65,118-125), all tensors in one launch.
 * jobs_device: DEVICE array (built once; blk0 = running sum of cavp_optimizer_blocks(n) over the preceding jobs, ascending).
 * kind 0 = SGD (m = momentum buffer, v unused), 1 = Adam (m, v = first / second moments, zero-initialised).
 * lr of a job = lr_sgd (or lr_adam) * lr_mult; step = 1 for the first call (SGD: buf = d; Adam bias corrections). */
typedef struct cavp_opt_job {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  float lr_mult;
  float weight_decay;
  int32_t blk0;
  int32_t kind;
  int32_t vec;   /* p, g, m 16-byte aligned: float4 path */
  int32_t pad_;
} cavp_opt_job;
int32_t cavp_optimizer_blocks(int64_t n);
int cavp_optimizer_step(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float lr_sgd, float lr_adam,
                        float momentum, float beta1, float beta2, float eps, int64_t step, void* stream);

/* Device-resident schedule (added to ABI 15): the step counter, the constants of the warm-up + poly schedule
 * (engine/lr_policy.py:30-43) and of Adam, and the scalars of the current step, so that the optimiser step needs nothing
 * from the host and can be recorded in a hipGraph.  The host fills t and the constants once; the device writes the rest.
 * cavp_optimizer_schedule (one thread) computes, in double precision and rounded to f32 once, the scalars of step t:
 *   lr_sgd = start_lr for t == 0, else get_lr(t - 1) (the reference sets the rate after the step), where get_lr(i) =
 *            start_lr * i / warmup_steps for i < warmup_steps, end_lr for i >= total_iters (outside the reference's domain),
 *            else clamp(start_lr * (1 - i / total_iters) ^ lr_power, end_lr, start_lr);
 *   lr_adam = base_lr;  bc1 = 1 - beta1^(t+1);  bc2_sqrt = sqrt(1 - beta2^(t+1));  first_step = (t == 0);
 * and then stores t + 1.  cavp_optimizer_step_dev is cavp_optimizer_step with those scalars loaded from the state block;
 * issue it behind the schedule launch on the same stream.  Neither launch synchronises or touches host memory. */
typedef struct cavp_opt_state {
  int64_t t;            /* completed steps */
  int64_t total_iters;
  int64_t warmup_steps;
  double start_lr;
  double lr_power;
  double end_lr;
  float base_lr;        /* Adam's constant rate */
  float beta1;
  float beta2;
  float lr_sgd;         /* from here on: written by the device */
  float lr_adam;
  float bc1;
  float bc2_sqrt;
  int32_t first_step;
} cavp_opt_state;
int64_t cavp_optimizer_state_bytes(void);
int cavp_optimizer_schedule(cavp_opt_state* state_device, void* stream);
int cavp_optimizer_step_dev(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum, float eps,
                            const cavp_opt_state* state_device, void* stream);

/* Step guard (added to ABI 16): global gradient norm, clip_grad_norm_ clipping, a skip of the whole update when a gradient is
 * not finite, and a ring of per-step records, all on the device so that a captured iteration needs no host value for them.
 * One guarded step is four launches on one stream, each ordered behind the one before it by the stream alone:
 *   cavp_grad_guard_partials -> cavp_grad_guard_finish -> cavp_optimizer_schedule_guarded -> cavp_optimizer_step_guarded.
 * The host fills max_norm, skip_nonfinite and history (and zeroes the rest) once; the device writes everything else.
 * The ring of `history` cavp_step_record follows the state block directly, at byte offset cavp_guard_state_bytes(). */
typedef struct cavp_guard_state {
  float max_norm;          /* <= 0: no clipping */
  int32_t skip_nonfinite;  /* CAVP_GUARD_SKIP_* bits; 0: never skip */
  int32_t history;         /* capacity of the record ring, >= 1 */
  int32_t skip;            /* from here on: written by the device, every step */
  float grad_norm;         /* 2-norm over every gradient the update reads */
  float norm_sgd;          /* ... over the kind 0 jobs */
  float norm_adam;         /* ... over the kind 1 jobs */
  float clip_coef;         /* max_norm > 0 ? min(1, max_norm / (grad_norm + 1e-6)) : 1 (torch's clip_grad_norm_) */
  int64_t nonfinite;       /* gradient elements that are NaN or +-inf */
  int64_t skipped_total;
  int64_t head;            /* records written so far; record i lives in slot i % history */
} cavp_guard_state;
#define CAVP_GUARD_SKIP_GRADIENTS 1   /* skip the update when a gradient element or the norm is not finite (the finish launch) */
#define CAVP_GUARD_SKIP_LOSSES 2      /* ... and when a loss handed to the schedule launch is not finite; the losses are the caller's
                                         and, data parallel, must be equal on every rank (the gradients are: the arena is reduced) */
#define CAVP_STEP_SKIPPED 1      /* cavp_step_record.flags */
#define CAVP_STEP_CLIPPED 2      /* clip_coef < 1 */
#define CAVP_STEP_NO_LOSS 4      /* no loss pointer was given: l_ce is 0 */
#define CAVP_STEP_NO_LOSS1 8     /* no second loss pointer was given: l_ctr is 0 */
#define CAVP_STEP_SKIPPED_LOSS 16 /* skipped (also) because a loss was not finite */
typedef struct cavp_step_record {
  int64_t t;               /* the step index this update ran as; on a skip, the one that did not run */
  int64_t nonfinite;
  float l_ce;
  float l_ctr;
  float lr_sgd;            /* the SGD rate of step t */
  float grad_norm;
  float clip_coef;
  int32_t flags;
} cavp_step_record;
typedef struct cavp_guard_partial {
  float sumsq;
  int32_t nonfinite;
} cavp_guard_partial;
int64_t cavp_guard_state_bytes(void);
int64_t cavp_step_record_bytes(void);
/* One workgroup per optimiser block (4096 elements, the update's own block -> job mapping): partials[block] = the f32 sum of
 * squares (a 12-level tree, no chain) and the non-finite count of that block's gradients.  No atomics, every block writes its slot,
 * the arena is read once.  partials: total_blocks entries. */
int cavp_grad_guard_partials(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, cavp_guard_partial* partials,
                             void* stream);
/* One workgroup: per job the partials in a fixed lane order, then the jobs in a fixed order, all in double; then grad_norm,
 * norm_sgd, norm_adam, nonfinite, clip_coef (from the norm in double, rounded once) and
 * skip = (skip_nonfinite & CAVP_GUARD_SKIP_GRADIENTS) && (nonfinite > 0 || !isfinite(grad_norm)). */
int cavp_grad_guard_finish(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                           const cavp_guard_partial* partials, cavp_guard_state* guard_device, void* stream);
/* One thread.  guard->skip: the state block is left as it is (t, rates, bias corrections, first_step) and skipped_total grows by one;
 * otherwise cavp_optimizer_schedule's arithmetic (one shared device function).  With CAVP_GUARD_SKIP_LOSSES a given loss that is NaN or
 * +-inf sets guard->skip here as well, and CAVP_STEP_SKIPPED_LOSS in the record (the CE head answers "every label ignored" with a NaN loss and zero gradients).  Either way the record of this step is written to
 * slot head % history and head grows by one.  loss0 / loss1: optional 1-element f32 device arrays (NULL: 0 and the flag). */
int cavp_optimizer_schedule_guarded(cavp_opt_state* state_device, cavp_guard_state* guard_device, const float* loss0,
                                    const float* loss1, void* stream);
/* cavp_optimizer_step_dev with the gradient taken as clip_coef * g; every workgroup returns at once when guard->skip.  The
 * gradient arena is NOT rescaled (torch.nn.utils.clip_grad_norm_ scales p.grad in place; here p.grad keeps the raw gradient). */
int cavp_optimizer_step_guarded(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum, float eps,
                                const cavp_opt_state* state_device, const cavp_guard_state* guard_device, void* stream);

/* Gradient accumulation (added to ABI 16): n micro-batches per optimiser update, with nothing taken from the host, so that the
 * captured step can run "7 of 8 replays only accumulate, the 8th also guards, schedules and updates".  The accumulator is a flat
 * f32 buffer with the gradient arena's layout (an element lives at its gradient's offset from arena_base; both bases 16-byte
 * aligned, the accumulator at least as long as the arena).  One micro-step is, on one stream:
 *   cavp_grad_accumulate -> cavp_accum_advance -> the gated twins of the optimiser's launches, in the ungated order.
 * The host fills n (>= 1) and k (the index of the next micro-step in its window, 0 <= k < n) and zeroes the rest. */
typedef struct cavp_accum_state {
  int32_t n;             /* micro-steps per window */
  int32_t k;             /* index of the next micro-step in the window */
  int32_t gate;          /* from here on: written by the device.  1 while the current micro-step closes a window */
  int32_t pad_;
  int64_t windows;       /* windows closed so far */
  int64_t micro_total;   /* micro-steps so far */
  float loss_sum0;       /* running f32 sums of the two loss words over the window, in micro-step order */
  float loss_sum1;
  float loss_mean0;      /* the last closed window's means: sum / n, correctly rounded */
  float loss_mean1;
} cavp_accum_state;
int64_t cavp_accum_state_bytes(void);
/* One workgroup per optimiser block (the update's job table and block map).  With g the gradients in the arena and k, n loaded
 * from the state block: k == 0: acc <- g (a copy; the accumulator is not read);  0 < k < n - 1: acc <- acc + g;
 * k == n - 1: g <- acc + g (the window's sum goes back into the arena);  n == 1: returns at once.  One IEEE f32 add per element
 * and micro-step.  Reads the state block only; no atomics, no workgroup depends on another.  Gradients outside the job table
 * and the padding between views are not touched. */
int cavp_grad_accumulate(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, const float* arena_base,
                         float* acc_base, const cavp_accum_state* state_device, void* stream);
/* One thread, behind the accumulate launch: gate = (k == n - 1); for each given loss word sum = (k == 0 ? l : sum + l) and, when
 * the window closes, mean = sum / n; then k = (k + 1) mod n, micro_total + 1, windows + gate.  loss0 / loss1: optional 1-element
 * f32 device arrays. */
int cavp_accum_advance(cavp_accum_state* state_device, const float* loss0, const float* loss1, void* stream);
/* Gated twins of the six device-schedule launches above: gate_device points at cavp_accum_state.gate.  Zero: every workgroup
 * returns at once and nothing is written (no record, no skipped_total, t, rates, parameters and state buffers untouched);
 * otherwise the ungated launch's device code runs, so equal states give equal bits. */
int cavp_optimizer_schedule_gated(cavp_opt_state* state_device, const int32_t* gate_device, void* stream);
int cavp_optimizer_step_dev_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum, float eps,
                                  const cavp_opt_state* state_device, const int32_t* gate_device, void* stream);
int cavp_grad_guard_partials_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                   cavp_guard_partial* partials, const int32_t* gate_device, void* stream);
int cavp_grad_guard_finish_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks,
                                 const cavp_guard_partial* partials, cavp_guard_state* guard_device, const int32_t* gate_device,
                                 void* stream);
int cavp_optimizer_schedule_guarded_gated(cavp_opt_state* state_device, cavp_guard_state* guard_device, const float* loss0,
                                          const float* loss1, const int32_t* gate_device, void* stream);
int cavp_optimizer_step_guarded_gated(const cavp_opt_job* jobs_device, int32_t njobs, int32_t total_blocks, float momentum,
                                      float eps, const cavp_opt_state* state_device, const cavp_guard_state* guard_device,
                                      const int32_t* gate_device, void* stream);

/* Step rollback (added to ABI 16): a skipped step also undoes what its forward wrote.  A device-resident table of byte ranges, two
 * launches whatever the number of ranges:
 *   cavp_rollback_save:    live -> shadow for every range without CAVP_ROLLBACK_SCRUB;
 *   cavp_rollback_restore: loads word_device[0] (the step guard's cavp_guard_state.skip; NULL = forced).  Zero: every workgroup returns
 *                          after that one load.  Otherwise shadow -> live for every range, zeros into the CAVP_ROLLBACK_SCRUB ranges.
 * A range is `nbytes` bytes (a multiple of 4) at any 4-byte aligned live / shadow address; copies are 16-byte vectors where the
 * two addresses share their offset from a 16-byte boundary and the vector lies inside the range, dwords elsewhere; nothing outside
 * [live, live + nbytes) and [shadow, shadow + nbytes) is read or written.  Live ranges must not overlap each other or a shadow.
 * Work units: a range is cut into blocks of 1024 bytes on a grid that starts at the 16-byte boundary at or below `live`, that is
 * cavp_rollback_blocks(live_address, nbytes) = ceil(((live_address & 15) + nbytes) / 1024) blocks; blk0 = the running sum over the
 * preceding ranges (ascending), total_blocks = the sum over all.  A workgroup serves 16 consecutive blocks whatever ranges they belong
 * to (many small ranges share one), the grid is min(ceil(total_blocks / 16), 2048) workgroups striding over the rest.
 * The state block counts the launches that did something: saves, and restores whose word was set or that were forced (the only
 * atomics).  nranges == 0 or total_blocks == 0: success, nothing launched, nothing counted. */
typedef struct cavp_rollback_range {
  void* live;
  void* shadow;            /* NULL for a scrub range */
  int64_t nbytes;
  int32_t blk0;
  int32_t flags;           /* CAVP_ROLLBACK_* */
} cavp_rollback_range;
#define CAVP_ROLLBACK_SCRUB 1   /* not saved; zero-filled by a restore that happens */
typedef struct cavp_rollback_state {
  int64_t saves;
  int64_t restores;
} cavp_rollback_state;
int64_t cavp_rollback_range_bytes(void);
int64_t cavp_rollback_state_bytes(void);
int64_t cavp_rollback_blocks(int64_t live_address, int64_t nbytes);
int cavp_rollback_save(const cavp_rollback_range* table_device, int32_t nranges, int32_t total_blocks,
                       cavp_rollback_state* state_device, void* stream);
int cavp_rollback_restore(const cavp_rollback_range* table_device, int32_t nranges, int32_t total_blocks,
                          const int32_t* word_device, cavp_rollback_state* state_device, void* stream);

/* ---- log-mel front-end = trainers' preprocess_audio (trainer_cavp_vpo_mono.py:43-52,59-69;
 * utils/sourcesep.py:23-47): STFT(n_fft 512, hop, centred window, reflect padding) -> |.|^2 -> mel filterbank ->
 * 20 log10(max(amin, x)) -> 2 (x - spec_min) / (spec_max - spec_min) - 1.
 * wave: f32 [N][A]; window: f32 [n_fft] (Hann of win_length, zero-padded to the frame centre); fb: f32 [n_fft/2+1][n_mels];
 * out: f32 [N][n_frames][n_mels] (n_frames <= 1 + A / hop). */
int cavp_mel_frontend(const float* wave, int32_t N, int32_t A, const float* window, const float* fb, float* out,
                      int32_t n_fft, int32_t hop, int32_t n_frames, int32_t n_mels, float amin, float spec_min,
                      float spec_max, void* stream);

/* ---- pixel-level audio-visual InfoNCE (loss/contrastive_aud.py::ContrastLoss, config #5 / SURVEY.md §8a row a13) ----
 * The class-balanced sampling (torch.randperm on the CPU generator, contrastive_aud.py:76-141) stays on the host; these
 * are the device stages for the N sampled anchors.  S = A A^T / T and dA = G A run on cavp_conv2d_nhwc / _wgrad. */
/* Nearest-neighbour down-sampling of the int64 label maps [B][H][W] to the feature resolution, int32 [B][h][w]
 * (contrastive_aud.py:18-22 `F.interpolate(gt.unsqueeze(1).float(), size, mode='nearest')`): only B*h*w int32 labels travel to the
 * host for the class-balanced sampling instead of the full-resolution int64 maps. */
int cavp_label_nearest(const int64_t* gt, int32_t* out, int32_t B, int32_t H, int32_t W, int32_t h, int32_t w, void* stream);
/* The chain's kernels take the anchor count from `header` on the device (the device sampler's plan below: n = clamp(header[0], 0,
 * cap), n_match = header[1]; N / n_match ignored, cap > 0) or, header == NULL, from the host: (N, n_match), N > 0,
 * 0 <= n_match <= N.  Index and label arrays hold at least cap rows with a header, at least N without.  Rows < n_match read /
 * write the match tensor, the others the shuffle one. */
/* A[i] = x[b_i, :, p_i] / max(||.||, eps); xm / xs addressed by element strides (works for NCHW memory and for the NHWC
 * memory behind out_fusion); also saves the norms (F.normalize, contrastive_aud.py:25-26 + gathers :97-139).  rows (>= cap
 * resp. N, the leading dimension of A / S): rows >= n of A are zero-filled, norms 1. */
int cavp_gather_l2norm(const float* xm, int64_t m_stride_b, int64_t m_stride_c, int64_t m_stride_p, const float* xs,
                       int64_t s_stride_b, int64_t s_stride_c, int64_t s_stride_p, const int32_t* header, const int32_t* idx_b,
                       const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match, int32_t rows, int32_t C, float eps, float* A,
                       float* norms, void* stream);
/* info_nce (contrastive_aud.py:41-74) on S[ld][ld] (already / temperature; ld >= cap resp. N): row_mlpp[i], loss[0] =
 * -mean(row_mlpp), 0 when n == 0; columns / rows >= n of S are ignored; optional dS = grad_scale * dloss/dS, zero outside [n][n]. */
int cavp_infonce_rows(const float* S, const int32_t* labels, const int32_t* header, int32_t cap, int32_t N, int32_t ld, float eps,
                      float* row_mlpp, float* loss, float* dS, float grad_scale, void* stream);
/* g = (d + d^T) * scale * (scale_dev ? scale_dev[0] : 1): the loss's upstream gradient (a device scalar in torch.autograd) stays on
 * the device - reading it on the host stalled the launch queue behind the whole forward pass (config #5,
 * trainer_cavp_vpo_mono.py:178-190) */
int cavp_symm_add(const float* d, float* g, int32_t n, float scale, const float* scale_dev, void* stream);
/* dx[b_i, :, p_i] = (dA_i - A_i <A_i, dA_i>) / norms[i] for the rows < n; nothing else of dxm / dxs is written. */
int cavp_l2norm_bwd_scatter(const float* dA, const float* A, const float* norms, const int32_t* header, const int32_t* idx_b,
                            const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match, int32_t C, float* dxm, int64_t m_stride_b,
                            int64_t m_stride_c, int64_t m_stride_p, float* dxs, int64_t s_stride_b, int64_t s_stride_c,
                            int64_t s_stride_p, void* stream);

/* ---- ABI 14: device-side anchor sampling (opt-in; contrastive_aud.py:76-141 with a counter-based generator) ----
 * The selection rule of extraction_samples with Philox4x32-10 in place of torch.randperm, so that the whole loss step runs
 * without the host and can be captured in a hipGraph.  Pixel i = b*HW + p of the reduced label map has the 64-bit keys
 *   key(stream, i) = (r0 << 32) | r1,  r = Philox4x32-10(counter = (i, stream, offset_lo, offset_hi), key = (seed_lo, seed_hi)),
 * stream 0 = per-class pick, 1 = background, 2 = shuffle candidates; "pick q of a group" = its q members with the smallest
 * (key, i), in ascending (key, i).  Rows: every kept class ascending (max_views each, label c), sample_num background pixels
 * (label 0), sample_num of all match-foreground pixels (label gs[i]); sample_num = min(max_views, n_fg, n_bg); n = 0 when no class
 * has max_views pixels.  Of more than max_classes qualifying classes the lowest-numbered are kept.
 *   state  int64[4] (device, persistent): {seed, offset, dropped_classes, bad_labels}; a call reads seed / offset, then
 *          offset += 1, dropped_classes += surplus classes, bad_labels += labels outside [0, 255] (such a pixel is in no group).
 *   header int32[8]: {n, n_match, k_kept, sample_num, offset_lo, offset_hi, seed_lo, seed_hi} of this call.
 *   work   cavp_contrast_sample_work_bytes(max_classes) bytes of scratch; idx_b / idx_p / labels: int32[cap], cap =
 *          (max_classes + 2) * max_views; rows >= n are filled with -1.
 * 1 <= max_views <= 1024, 1 <= max_classes <= 254, total = B*HW < 2^31.  Deterministic for a given (seed, offset). */
size_t cavp_contrast_sample_work_bytes(int32_t max_classes);
int cavp_contrast_sample(const int32_t* gm, const int32_t* gs, int64_t total, int32_t HW, int32_t ignore_idx, int32_t max_views,
                         int32_t max_classes, int64_t* state, int32_t* header, int32_t* work, int32_t* idx_b, int32_t* idx_p,
                         int32_t* labels, void* stream);

/* ---- The two ends of the chain on the training tape's fusion map (two entry points added to ABI 15; nothing else changed) ----
 * x / g: the map as it lies in memory, [2B][HW][ld] of `dtype` (CAVP_F32 / CAVP_BF16), ld >= C, the match half first.  Anchor row i
 * addresses image idx_b[i] (i < n_match) or B + idx_b[i] (i >= n_match), pixel idx_p[i].  The anchor count comes from `header`
 * (the device sampler's, cap = the plan's capacity) or, header == NULL, from (N, n_match).  One wave per row, 16-byte vectors,
 * f32 arithmetic.  C % 8 == 0 and ld a multiple of the 16-byte vector, else CAVP_ERR_BAD_ARG; x / g / A / dA 16-byte aligned.
 * A plan entry outside [0, B) x [0, HW) counts as a row >= n. */
/* A[i] = x_row / max(||x_row||_2, eps) as f32 [rows][C] + norms[i]; rows (>= cap resp. N): rows >= n are zero with norm 1. */
int cavp_contrast_gather_nhwc(int32_t dtype, const void* x, int32_t B, int32_t HW, int32_t ld, int32_t C, const int32_t* header,
                              const int32_t* idx_b, const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match, int32_t rows,
                              float eps, float* A, float* norms, void* stream);
/* g_row += scale * (dA_i - A_i <A_i, dA_i>) / norms[i], read-modify-write in `dtype`, no atomics: the anchors must be distinct
 * pixels per half (both samplers pick without replacement).  Rows outside the plan and channels >= C are not touched. */
int cavp_contrast_rows_bwd_add(int32_t dtype, void* g, int32_t B, int32_t HW, int32_t ld, int32_t C, const int32_t* header,
                               const int32_t* idx_b, const int32_t* idx_p, int32_t cap, int32_t N, int32_t n_match, const float* dA,
                               const float* A, const float* norms, float scale, void* stream);

/* ---- PVTv2-B5 visual backbone (models/visual/backbones/pvt/pvt.py, config #4 / SURVEY.md §8a row a12) ---- */
/* Attention.forward (pvt.py:102-130): softmax(q k^T * scale) v per head with the spatially-reduced K/V (Nk <= 256,
 * head_dim 64).  q, o: [B][Nq][heads*64]; kv: [B][Nk][2*heads*64] (k then v, as written by the `kv` Linear). */
int cavp_sra_attention(int32_t dtype, const void* q, const void* kv, void* o, int32_t B, int32_t Nq, int32_t Nk,
                       int32_t heads, int32_t head_dim, float scale, void* stream);
/* DWConv (pvt.py:315-326): depth-wise 3x3 pad 1 + bias on NHWC, optional fused act (GELU of Mlp.forward :46-55). */
int cavp_dwconv3x3_nhwc(int32_t dtype, const void* x, const float* w9c, const float* bias, void* y, int32_t N, int32_t H,
                        int32_t W, int32_t C, int32_t act, void* stream);
/* ABI 7: the same with act = CAVP_ACT_GELU and gelu'(t) stored into aux (y's shape; NULL = plain call): what the backward of
 * Mlp.forward (pvt.py:46-55) needs - it is multiplied into the data-gradient GEMM of fc2 (cavp_conv_desc.aux_mode 2), so the
 * training pass has no separate GELU and GELU-backward launches and the pre-activation is never stored. */
int cavp_dwconv3x3_nhwc_aux(int32_t dtype, const void* x, const float* w9c, const float* bias, void* y, void* aux, int32_t N,
                            int32_t H, int32_t W, int32_t C, int32_t act, void* stream);
/* data gradient of the depth-wise conv (pvt.py:46-55 backward): dx = dy correlated with the reversed taps of the same packed
 * [9][C] weights; dense NHWC of C channels. */
int cavp_dwconv3x3_bwd_data_nhwc(int32_t dtype, const void* dy, const float* w9c, void* dx, int32_t N, int32_t H, int32_t W,
                                 int32_t C, void* stream);
int cavp_pack_dwconv_weight(const float* w_c133, float* w9c, int32_t C, void* stream); /* [C][1][3][3] -> [9][C] */
/* OverlapPatchEmbed.proj of stage 1 (pvt.py:187-188): KSxKS conv, Cin <= 3, NCHW f32 in, NHWC out, + bias. */
int cavp_conv_smallcin_kxk_nchw(int32_t dtype, const float* x_nchw, const float* w_oihw, const float* bias, void* y_nhwc,
                                int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t KS, int32_t stride,
                                int32_t pad, void* stream);

/* ---- PVTv2-B5 training pass (backward of the kernels above; pvt.py:102-130,46-55,187-188,167-168) ---- */
/* Attention backward: dq [B][Nq][heads*64] (dtype), dkv f32 [B][Nk][2*heads*64] (dk | dv; overwritten) from q, kv, dout.
 * The softmax is recomputed from q and kv (nothing is saved by the forward).  workspace: row statistics,
 * cavp_sra_attention_bwd_workspace_bytes(B, Nq, heads) bytes, 16-byte aligned. */
size_t cavp_sra_attention_bwd_workspace_bytes(int32_t B, int32_t Nq, int32_t heads);
int cavp_sra_attention_bwd(int32_t dtype, const void* q, const void* kv, const void* dout, void* dq, float* dkv, int32_t B,
                           int32_t Nq, int32_t Nk, int32_t heads, int32_t head_dim, float scale, void* workspace,
                           size_t workspace_bytes, void* stream);
/* same, with dkv written in `dkv_dtype` (CAVP_F32 / CAVP_BF16): the fixed-order sum of the query splits' partials stores the
 * consumer's dtype directly. */
int cavp_sra_attention_bwd_to(int32_t dtype, const void* q, const void* kv, const void* dout, void* dq, void* dkv,
                              int32_t dkv_dtype, int32_t B, int32_t Nq, int32_t Nk, int32_t heads, int32_t head_dim, float scale,
                              void* workspace, size_t workspace_bytes, void* stream);
/* DWConv weight / bias gradient: dw_c133 f32 [C][1][3][3] += , dbias f32 [C] += (may be NULL).  The data gradient is
 * cavp_dwconv3x3_nhwc with the taps reversed. */
int cavp_dwconv3x3_wgrad(int32_t dtype, const void* x, const void* dy, float* dw_c133, float* dbias, int32_t N, int32_t H,
                         int32_t W, int32_t C, void* stream);
/* weight / bias gradient AND data gradient of the depth-wise conv in one walk over dy (w9c: the forward's packed [9][C] taps;
 * dx: dense NHWC of x's dtype, overwritten).  w9c = dx = NULL: the weight gradient alone. */
int cavp_dwconv3x3_bwd(int32_t dtype, const void* x, const void* dy, const float* w9c, void* dx, float* dw_c133, float* dbias,
                       int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* Weight gradient of cavp_conv_smallcin_kxk_nchw, step 1: im2col of the NCHW f32 input into cols [N*Ho*Wo][Kpad] (dtype;
 * column order (ci, kh, kw) = the OIHW weight's, zero beyond Cin*KS*KS; Kpad a multiple of 8).  Step 2 is
 * cavp_conv2d_wgrad_nhwc as a 1x1 layer with x = cols, giving dw [Cout][Kpad]. */
int cavp_smallcin_kxk_im2col(int32_t dtype, const float* x_nchw, void* cols, int32_t N, int32_t Cin, int32_t H, int32_t W,
                             int32_t KS, int32_t stride, int32_t pad, int32_t Kpad, void* stream);
/* [B][H][W][C] -> [B][H/s][W/s][s*s*C] (inverse != 0: back): the spatial-reduction conv (kernel = stride = s,
 * pvt.py:76-79) becomes a token GEMM over the rearranged rows, forward and backward. */
int cavp_space_to_depth(int32_t dtype, const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s,
                        int32_t inverse, void* stream);
/* timm DropPath around a residual branch (pvt.py:167-168): out = x + sample_scale[b] * branch; x == NULL: the branch's
 * gradient sample_scale[b] * g.  per_sample = elements per batch item. */
int cavp_row_scale_add(int32_t dtype, const void* x, const void* branch, const float* sample_scale, void* out, int32_t B,
                       int64_t per_sample, void* stream);
/* DropPath factors drawn on the device (one entry point added to ABI 16; nothing else changed; opt-in, cavp_amd/droppath.py).
 * state: int64 {seed, offset} on the device, the 16-byte head of the frame augmentation's state block.  keep, inv_keep: f32 [n],
 * 1 - p and the f32 quotient 1 / keep of every branch with p > 0, in forward order.  out: f32 [n][B], dense.
 *   r = Philox4x32-10(counter = (b, k, offset_lo, offset_hi), key = (seed_lo, seed_hi));  u = (r[0] >> 8) * 2^-24
 *   out[k][b] = keep[k] + u >= 1 ? inv_keep[k] : 0      (the sum in f32: timm 0.4.9's floor(keep + rand) / keep)
 * then offset += 1.  One workgroup, plain stores, no host synchronisation: capturable.  n >= 1, B >= 1 and non-null pointers
 * (CAVP_ERR_BAD_ARG), n * B <= 2^20 (CAVP_ERR_UNSUPPORTED). */
int cavp_drop_path_draw(int64_t* state, const float* keep, const float* inv_keep, int32_t n, int32_t B, float* out, void* stream);

/* ---- ResNet-18 audio encoder (two entry points added to ABI 16; nothing else changed): the eval forward of the reference's non-VGG
 * AudioModel (audio_network.py:18-25: torchvision resnet18, conv1 in_plane -> 64, avgpool = AdaptiveMaxPool2d((1, 1)), fc 512 -> out).
 * Its sixteen 3x3 and three 1x1 convs run through cavp_conv2d_nhwc; csrc/audio_resnet.hip holds the two launches below. ----
 * conv1 (7x7, stride 2, pad 3, no bias) + folded bn1 (scale / shift, f32 [64]) + ReLU + MaxPool2d(3, 2, 1) in ONE launch: the stem map
 * [N][Hs][Ws][64], Hs = (H - 1) / 2 + 1, stays in LDS.  x f32 NCHW [N][Cin][H][W], Cin = 1 or 2 (else CAVP_ERR_UNSUPPORTED); w f32 OIHW
 * [64][Cin][7][7]; y dense NHWC [N][Hp][Wp][64] of dtype (f32 accumulation), Hp = (Hs - 1) / 2 + 1, 16-byte aligned.  Any H, W >= 1. */
int cavp_audio_stem_pool(int32_t dtype, const float* x_nchw, const float* w_oihw, const float* scale, const float* shift,
                         void* y_nhwc, int32_t N, int32_t Cin, int32_t H, int32_t W, void* stream);
/* x.amax over HW for NHWC x [N][HW][C] with row stride ldx; y [N][C] of the SAME dtype (a maximum needs no wider type), dense.  HW >= 1;
 * the running maximum starts at -inf.  N <= 65535. */
int cavp_global_maxpool_nhwc(int32_t dtype, const void* x, void* y, int32_t N, int32_t HW, int32_t C, int32_t ldx, void* stream);
/* ---- training of that encoder (four entry points added to ABI 16; nothing else changed) ----
 * conv1 alone, raw, with the BatchNorm tile statistics of its output in ONE launch: z dense NHWC [N][Hs][Ws][64] of dtype (f32
 * accumulation), 16-byte aligned, and tile_stats f32 [tiles][64][2] = (mean, M2 about that mean) of the values AS STORED in z over
 * tile t's rows [t * rows_per_tile, min((t + 1) * rows_per_tile, N * Hs * Ws)) of z viewed as [N * Hs * Ws][64] - the table
 * cavp_bn_finalize_tiles and cavp_bn_tiles_scale_shift_act consume.  cavp_audio_stem_train_layout gives tiles and rows_per_tile
 * (a band of k stem rows of the flattened N * Hs row index: rows_per_tile = k * Ws) and returns 1, or returns 0 where the launch does
 * not cover the shape (Cin not 1 or 2, Ws > 192, more than 2^31 - 1 output pixels): cavp_audio_stem_train then returns
 * CAVP_ERR_UNSUPPORTED and the caller runs cavp_conv_smallcin_kxk_nchw + cavp_col_tile_stats.  One workgroup owns a tile: no
 * atomics, bit-reproducible. */
int cavp_audio_stem_train_layout(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t* tiles, int32_t* rows_per_tile);
int cavp_audio_stem_train(int32_t dtype, const float* x_nchw, const float* w_oihw, void* z_nhwc, float* tile_stats, int32_t N,
                          int32_t Cin, int32_t H, int32_t W, void* stream);
/* AdaptiveMaxPool2d((1, 1)) with its winner: y [N][C] (x's dtype) and arg int32 [N][C] = the FIRST position i in [0, HW) (scan order
 * h * W + w) at which x[n][i][c] equals the maximum - torch's rule, also for NaN: a NaN input gives y = NaN and arg = the LAST NaN's
 * position.  x NHWC [N][HW][C] with row stride ldx.  N <= 65535. */
int cavp_global_maxpool_arg_nhwc(int32_t dtype, const void* x, void* y, int32_t* arg, int32_t N, int32_t HW, int32_t C, int32_t ldx,
                                 void* stream);
/* its backward: dx dense [N][HW][C] (dtype), EVERY element written: dx[n][i][c] = arg[n][c] == i ? dy[n][c] : 0.  dy dense [N][C]. */
int cavp_global_maxpool_bwd_nhwc(int32_t dtype, const int32_t* arg, const void* dy, void* dx, int32_t N, int32_t HW, int32_t C,
                                 void* stream);

/* ---- validation metrics (ABI 13; utils/eval_utils.py MIoU / ForegroundDetect, utils/avsbench_utils.py mask_iou / Eval_Fmeasure) ----
 * Integer counts only, accumulated with integer atomics: results are independent of arrival order.  The float finalisation stays
 * on the host side (cavp_amd/metrics.py), in the reference's expressions.  None of these clears its output (cavp_zero_bytes). */
#define CAVP_METRICS_MAX_CLASSES 4096
#define CAVP_FMEASURE_MAX_THRESHOLDS 4096
/* M[row][p] += 1 ((K+1) x K, u64) for every pixel of f32 NCHW logits [N][C][HW] (dense; any 4-byte aligned base) with label
 * t = labels[n][hw] (dense [N][HW]; label_dtype CAVP_I64, or CAVP_F32 holding integers - a non-finite one is not counted) where
 * t >= 0 and t != ignore: p = argmax_c (first maximal index, a NaN counts as the maximum, as torch.max), row = t < K ? t : K.
 * MIoU's inter / union / correct / labeled and ForegroundDetect's confusion matrix (M[:K]) follow exactly.  K >= C.  16-byte
 * loads when HW % 4 == 0 and both bases are 16-byte aligned. */
int cavp_seg_confusion_nchw(const float* logits, const void* labels, int32_t label_dtype, int32_t N, int32_t C, int64_t HW,
                            int32_t K, int64_t ignore, uint64_t* M, void* stream);
/* out[n][0..3] += (sum p*t, sum max(p, t), sum (1-t)*(1-p), sum t) over the HW pixels of image n; pred / target dense [N][HW] of
 * CAVP_I64 or CAVP_F32 (f32 values must be integers, i.e. masks: they are converted to int64 per pixel). */
int cavp_mask_iou_stats(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t N, int64_t HW,
                        int64_t* out, void* stream);
/* hist[n][0][b] / hist[n][1][b] += pixels of image n with bin b = #{i < pr_num : thresholds[i] <= p}, over all pixels / over
 * gt != 0 (gt dense [N][HW], CAVP_F32 or CAVP_I64); thresholds ascending.  C == 0: src is a probability map whose image n is the
 * dense plane src + n * src_image_stride (>= HW; e.g. torch.softmax(logits, 1)[:, 1], stride C * HW); C >= 2: src is f32 logits,
 * image n = src + n * src_image_stride (>= C * HW) as [C][HW], and p = softmax over C, channel `channel`.
 * hist: u32 [N][2][pr_num + 1]. */
int cavp_fmeasure_hist(const float* src, int64_t src_image_stride, const void* gt, int32_t gt_dtype, const float* thresholds, int32_t N, int32_t C,
                       int32_t channel, int64_t HW, int32_t pr_num, uint32_t* hist, void* stream);

/* ---- ABI 15: segmentation mask, probability map and confusion counts straight from the low-resolution logits ----
 * x: NHWC logits [N][Hi][Wi][C] (dtype CAVP_F32 / CAVP_BF16, pixel pitch ldx >= C elements: a channel slice of a padded buffer is
 * fine).  Every output pixel (n, ho, wo) of the Ho x Wo grid gets its C bilinearly interpolated logits - the same taps, weights
 * and blend, hence the same f32 bits, as the cavp_bilinear_nhwc_to_nchw output - but that [N][C][Ho][Wo] tensor is never
 * written.  Outputs, each optional (NULL = skipped), at least one required:
 *   mask   u8  [N][Ho][Wo]: argmax over C (first maximal index, a NaN counts as the maximum, as torch.max).  Needs C <= 256.
 *   prob   f32 [N][Ho][Wo]: softmax over the C interpolated logits (max-subtracted), channel `channel` (0 <= channel < C).
 *   M      (K+1) x K u64 counts, together with `labels` (dense [N][Ho][Wo]; label_dtype CAVP_I64, or CAVP_F32 holding integers):
 *          M[row][p] += 1 with the bin rule of the NCHW confusion entry point above: p = the argmax, label t counted when t >= 0
 *          and t != ignore, row = t < K ? t : K; K >= C.  Not cleared here.  `labels` and `M` come together.
 * Any Hi, Wi -> Ho, Wo; the x4 ratio of the model head is the fast case (4 neighbouring pixels share 3 source columns).  16-byte
 * channel loads when ldx is a multiple of the 16-byte vector and x is 16-byte aligned, scalar loads otherwise; per-pixel arrays
 * take vector accesses when Wo % 4 == 0 and their base is aligned (mask 4, prob / labels 16 bytes).  No allocation, no sync. */
int cavp_seg_predict_nhwc(int32_t dtype, const void* x, int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t ldx, int32_t Ho,
                          int32_t Wo, int32_t align_corners, uint8_t* mask, float* prob, int32_t channel, const void* labels,
                          int32_t label_dtype, int32_t K, int64_t ignore, uint64_t* M, void* stream);

/* ---- Pair builder (four entry points added to ABI 15; nothing else changed): the mismatched audio-visual pairs of the reference
 * trainers (trainer_cavp_vpo_mono.py:87-115,148-181, SoundBank in models/cavp_model.py:21-52) without the host ----
 * A batch of B mono clips waveform [B][A] f32 with image labels img_label [B][K] i64 (multi-hot in {0, 1}, column 0 = background)
 * and a per-class FIFO of clips kept as a ring: bank [K][S][A] f32 + head int32[K], logical slot j = physical (head + j) % S,
 * slot 0 the oldest; a zeroed bank with zero heads is the empty FIFO.  Launch order on one stream: plan, gather, bank_update,
 * labels.  gather must precede bank_update: the slot an overwritten row reads is the one a push to that class replaces.
 *
 * cavp_pairs_plan (one workgroup; B <= 1024, K <= 256):
 *   perm[j] = the row with the j-th smallest (key, i), key of row i = (r0 << 32) | r1 of Philox4x32-10(counter = (i, stream,
 *   offset_lo, offset_hi), key = (seed_lo, seed_hi)), stream 0; perm_in (int32[B], optional) replaces the draw.
 *   if_match[i] = all_k(img_label[i][k] == img_label[perm[i]][k]).  With overwrite != 0: of the n_false rows with if_match == 0
 *   the q = ow_table[n_false] with the smallest (rank, i) are picked (rank = the stream-1 key, or rank_in int32[B] >= 0); a picked
 *   row with exactly one non-zero non-background label c becomes a match: if_match = 1, img_label_shuffle[i] = img_label[i],
 *   source[i] = ~c, its clip = logical slot 0 of class c BEFORE this step's pushes.  Every other row: img_label_shuffle[i] =
 *   img_label[perm[i]], source[i] = perm[i].  Then, rows ascending, a row with exactly one non-zero non-background label c pushes
 *   its clip at the end of class c's FIFO; of more than S pushes to one class only the last S are written.
 *   ow_table int32[ow_table_len], ow_table_len > B: the host's int(n * ow_rate) for n = 0 .. (no float arithmetic on the device).
 *   state  int64[4] (device, persistent): {seed, offset, bad_inputs, reserved}; a call reads seed / offset, then offset += 1 and
 *          bad_inputs += the img_label entries outside {0, 1} (taken as "non-zero") + the perm_in entries outside [0, B)
 *          (replaced by the identity): no input value makes a kernel read or write out of bounds.
 *   header int32[8]: {n_false, q, rows overwritten, rows written to the bank, offset_lo, offset_hi, seed_lo, seed_hi}.
 *   src_table int32[2B]: row r of the 2B-clip output comes from waveform row e (e >= 0) or from physical bank slot ~e of the
 *          flattened [K*S] slots (e < 0); the first B entries are 0 .. B-1.  wr_table int32[B]: the physical slot row r is
 *          written to, or -1.  The plan kernel is the only reader and writer of `head`.
 * cavp_pairs_gather: out [2B][A] from src_table.  cavp_pairs_bank_update: the writer rows into their slots.  Both use 16-byte
 *   accesses when A % 4 == 0 and every base is 16-byte aligned, 4-byte accesses otherwise.
 * cavp_pairs_labels: label_shuffle[i] = if_match[i] ? pix_label[i] : 0 over HW i64 per row (16-byte accesses when HW % 2 == 0
 *   and both bases are aligned); unmatched rows are written without a read.
 * No allocation, no synchronisation, no host read of a device value: the four launches are capturable in a hipGraph. */
int cavp_pairs_plan(const int64_t* img_label, int32_t B, int32_t K, int32_t S, const int32_t* perm_in, const int32_t* rank_in,
                    int32_t overwrite, const int32_t* ow_table, int32_t ow_table_len, int64_t* state, int32_t* head,
                    int32_t* header, int32_t* perm, uint8_t* if_match, int64_t* img_label_shuffle, int32_t* source,
                    int32_t* src_table, int32_t* wr_table, void* stream);
int cavp_pairs_gather(const float* waveform, const float* bank, const int32_t* src_table, int32_t B, int32_t K, int32_t S, int32_t A,
                      float* out, void* stream);
int cavp_pairs_bank_update(const float* waveform, const int32_t* wr_table, int32_t B, int32_t K, int32_t S, int32_t A, float* bank,
                           void* stream);
int cavp_pairs_labels(const int64_t* pix_label, const uint8_t* if_match, int32_t B, int64_t HW, int64_t* label_shuffle, void* stream);

/* ---- Frame augmentation (three entry points added to ABI 15; nothing else changed): VisualAugmentation.train_aug of the reference
 * (dataset/<set>/visual/visual_aug.py) on raw decoded uint8 frames, PIL's arithmetic restated (tests/_augment_ref.py) ----
 * frames uint8 [B][Hs][Ws][3] and masks uint8 [B][Hs][Ws]: sample i sits in the top-left h x w corner of its staging slot,
 * (h, w) = sizes int32 [B][2] on the device; bytes outside the corner are never read.  Launch order on one stream: plan,
 * contrast_mean (only with jitter), render.  B <= 1024, crop H <= Hs, W <= Ws.
 *
 * params int32 [B][16], one row per sample (written by plan; params_in, optional, has the same layout and replaces the draws,
 * words 12 .. 15 of it are ignored):
 *   0 flip   1 scale index   2..5 order of the jitter operations (a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue)
 *   6, 7, 8 brightness / contrast / saturation factor (f32 bits)   9 hue shift, the uint8 added to H   10 crop top   11 crop left
 *   12, 13 scaled height / width   14 the contrast degenerate (rounded mean of L; written by render, -1 without jitter)
 *   15 non-zero: this sample was counted in bad_inputs
 * cavp_aug_plan (one workgroup): draws with Philox4x32-10, counter = (sample, stream, offset_lo, offset_hi), key = seed (the
 *   device sampler's convention); stream 0: r0 -> flip = u > 0.5, r1 -> scale index; 1: r0 -> one of the 24 orders, r1 ->
 *   brightness = 0.5 + u; 2: contrast, saturation; 3: r0 -> hue = -0.25 + 0.5 u, shift = trunc(hue * 255) mod 256; 4: top, left
 *   (u = (r >> 8) / 2^24; an index below n = (r * n) >> 32).  scales64: HOST int32 [n_scales], scale = value / 64, 32 <= value
 *   <= 256, n_scales <= 16.  Scaled size = floor(h * value / 64) (the reference's int(h * s), exact).  Pad as the reference
 *   writes it: if min(sh, sw) < min(H, W): right = max(H - sw, 0), bottom = max(W - sh, 0); top in [0, ph - H], left in [0, pw - W].
 *   identity != 0: the test-time path (no draw, scale 1, window at the origin).  state int64[4] (device): {seed, offset,
 *   bad_inputs, reserved}; a call reads seed / offset, then offset += 1 and bad_inputs += the samples with a staged size outside
 *   1 <= h <= Hs, 1 <= w <= Ws, an empty scaled image, a params_in field out of range or a padded image that cannot hold the
 *   crop; those are rendered from clamped values, nothing is read or written out of bounds.  near_tab int32 [B][H + W]: PIL's
 *   NEAREST source row / column (mirrored under flip) of every crop row / column, -1 in the pad.  lsum uint64 [B]: zeroed.
 * cavp_aug_contrast_mean: lsum[i] += sum of L over the whole scaled image of sample i after the operations in front of the
 *   contrast one (exact integer atomics: bit-reproducible).  max_scale64 = the largest entry of scales64 (sizes the grid).
 * cavp_aug_render: image f32 [B][3][H][W] = ((u8 / 255) - mean) / std, label int64 [B][H][W]; one 16 x 64 tile of the crop per
 *   workgroup, the horizontally resampled rows in LDS.  mean3 / std3 (f32) and fill3 (int32, 0 .. 255) are HOST arrays of 3.
 * No allocation, no synchronisation, no host read of a device value: the launches are capturable in a hipGraph. */
int cavp_aug_plan(const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* scales64,
                  int32_t n_scales, int32_t jitter, int32_t identity, const int32_t* params_in, int64_t* state, int32_t* params,
                  int32_t* near_tab, uint64_t* lsum, void* stream);
int cavp_aug_contrast_mean(const uint8_t* frames, const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t max_scale64,
                           const int32_t* params, uint64_t* lsum, void* stream);
int cavp_aug_render(const uint8_t* frames, const uint8_t* masks, const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t H,
                    int32_t W, const float* mean3, const float* std3, const int32_t* fill3, int32_t jitter, int32_t* params,
                    const int32_t* near_tab, const uint64_t* lsum, float* image, int64_t* label, void* stream);

/* ---- Frame augmentation, resize variant (three entry points added to ABI 16; the three above are unchanged): the reference's
 * resize_flag = True (dataset/avss/visual/visual_aug.py:31-35,71-72,81-82) - flip, random scale, jitter, then a second resize to
 * H x W (BICUBIC frame, NEAREST mask) in place of pad + crop; PIL's arithmetic, restated in tests/_augment_resize_ref.py ----
 * Launch order on one stream: plan_resize, contrast_mean (only with jitter; the entry point above, unchanged), resize_store,
 * resize_render.  The test-time path (identity != 0: resize, ToTensor, Normalize) is plan_resize, resize_render on the frames.
 * H x W may exceed the slot (an upscale).  The second pass holds 34 taps: floor(Hs * max_scale64 / 64) <= 8 H and the same for
 * the widths (identity: Hs <= 8 H, Ws <= 8 W), CAVP_ERR_UNSUPPORTED otherwise.
 * cavp_aug_plan_resize: the arguments, the params row and the draws of streams 0 .. 3 of the plan entry point above; stream 4 is not
 *   drawn, top = left = 0 (words 10, 11 of params_in are ignored), no sample is "too small"; bad_inputs counts staged sizes outside
 *   the slot, an empty scaled image and params_in fields out of range.  near_tab int32 [B][H + W]: the source row / column of every
 *   output row / column through both NEAREST walks (scaled -> output, source -> scaled), mirrored under flip.
 * cavp_aug_resize_store: scratch uint32 [B][mh][mw], mh = floor(Hs * max_scale64 / 64), mw likewise: the scaled, flipped, jittered
 *   image r | g << 8 | b << 16 in the top-left sh x sw corner of the sample's slot (the two-pass BICUBIC of the crop variant,
 *   rounded to uint8 after each pass); writes word 14 of the params row with jitter.
 * cavp_aug_resize_render: the second two-pass BICUBIC from src - the scratch (src_is_frames == 0) or, for the test-time path, the
 *   staged frames themselves (src_is_frames != 0, source size = sizes) - to image f32 [B][3][H][W] = ((u8 / 255) - mean) / std and
 *   label int64 [B][H][W] through near_tab; one 16 x 64 output tile per workgroup, at most 154 horizontally resampled rows in LDS.
 * No allocation, no synchronisation, no host read of a device value: the launches are capturable in a hipGraph. */
int cavp_aug_plan_resize(const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* scales64,
                         int32_t n_scales, int32_t jitter, int32_t identity, const int32_t* params_in, int64_t* state, int32_t* params,
                         int32_t* near_tab, uint64_t* lsum, void* stream);
int cavp_aug_resize_store(const uint8_t* frames, const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t max_scale64,
                          int32_t jitter, int32_t* params, const uint64_t* lsum, uint32_t* scratch, void* stream);
int cavp_aug_resize_render(const void* src, int32_t src_is_frames, const uint8_t* masks, const int32_t* sizes, int32_t B, int32_t Hs,
                           int32_t Ws, int32_t max_scale64, int32_t H, int32_t W, const float* mean3, const float* std3,
                           const int32_t* params, const int32_t* near_tab, float* image, int64_t* label, void* stream);

/* ---- Label stage (three entry points added to ABI 16; nothing else changed): the image labels the reference's data sets compute from
 * the mask after the transform (vpo_mono/multi_source/visual/visual_dataset.py:127-145, avss/visual/visual_dataset.py:157-165,
 * avsbench_ms.py:135-136), restated in tests/_labels_ref.py ----
 * label: B images of HW pixels, contiguous, int64 (label_u8 == 0) or uint8 (label_u8 != 0); never written.  Launch order on one
 * stream: presence (only with a remap), scan, expand.  B <= 1024, K <= 256.  16-byte loads when the base is 16-byte aligned and
 * HW % 2 == 0 (int64) resp. HW % 16 == 0 (uint8), element loads otherwise.
 *
 * mask, raw_mask uint32 [B][8] (device, persistent): bit v of image b; both must be ZERO before the first call and are left zero by
 *   the expand launch, so nothing is cleared outside the launches.
 * presence: raw_mask[b] |= the values in [0, 256) of image b.
 * scan, per pixel value v, in this order:
 *   remap (int32 [256] on the device, optional): the reference's loop "for i in unique(label) without 0 and ignore, ascending:
 *     label[label == i] = remap[i]" runs in place over a value list taken before the loop, so a pixel moved to t > i moves again at
 *     step t when t was in the raw image.  Per pixel: x = v; t = remap[x]; while t > x, t in the raw image, t not 0 and not ignore:
 *     x = t, t = remap[x]; the result is t.  remap[x] outside [0, 255] (-1 = "the reference raises"): the pixel keeps x and is bad.
 *     A v outside [0, 256) is no key of the table: it is kept and is bad unless it equals ignore.
 *   class bit, any_foreground == 0: mask[b] bit f for the result f in [0, K) and != ignore; f outside [0, K) and != ignore: bad, no bit.
 *              any_foreground != 0 (K == 2): bit 1 for every f != 0 (ignore included, as in the reference's sum).
 *   binary != 0: f != 0 and f != ignore becomes 1 (after the class bit, as in the AVSS data set).
 *   out_label int64 [B][HW] (optional): the value after these steps.  state int64[4] (device, persistent): state[0] += the pixels
 *   that were bad by at least one rule; no value makes a kernel read or write out of bounds.
 * expand: img_label int64 [B][K] = the bits (any_foreground: {1, 0} without bit 1, {0, 1} with it); clears mask and raw_mask (NULL
 *   without a remap).
 * No allocation, no synchronisation, no host read of a device value: the launches are capturable in a hipGraph. */
int cavp_labels_presence(const void* label, int32_t label_u8, int32_t B, int64_t HW, uint32_t* raw_mask, void* stream);
int cavp_labels_scan(const void* label, int32_t label_u8, int32_t B, int64_t HW, int32_t K, int32_t any_foreground,
                     const int32_t* remap, int32_t binary, int64_t ignore, const uint32_t* raw_mask, uint32_t* mask, int64_t* state,
                     int64_t* out_label, void* stream);
int cavp_labels_expand(uint32_t* mask, uint32_t* raw_mask, int32_t B, int32_t K, int32_t any_foreground, int64_t* img_label,
                       void* stream);

/* ---- Clip validation (two entry points added to ABI 16; nothing else changed): the validation loop of the AVSS trainers
 * (trainer_cavp_avss_image.py:295-349) for a batch of B clips of T frames at once, restated in tests/_clipval_ref.py ----
 * Frame n = b * T + t takes part iff t < clamp(count[b], 0, T) (count: device int32 [B], or int64 with count_i64 != 0; NULL: all
 * frames).  A frame that does not take part is not read.  Every pixel of a participating frame has a label v (labels: dense int64
 * [B*T][HW], never written) and a prediction p: pred_is_mask == 0: pred is dense f32 logits [B*T][C][HW] (any 4-byte aligned
 * base), p = argmax over C (first maximal index, a NaN counts as the maximum); pred_is_mask != 0: pred is a dense u8 class mask
 * [B*T][HW] (C is ignored).  16-byte loads when HW % 4 == 0 and the bases are aligned (mask: 4 bytes), element loads otherwise.
 *
 * cavp_clipval_frame_counts adds, per participating frame, into the per-frame scratch (u32, u32 atomics):
 *   hist[n][256]      the label histogram: bin v for 0 <= v < 256, bin `ignore` for v < 0;
 *   conf[n][(K+1)*K]  the confusion counts with the bin rule of the NCHW confusion entry point above (v < 0 or v == ignore: no
 *                     count; row = v < K ? v : K).
 *   A pixel with v >= 256 or with a mask byte p >= K is counted in state[0] resp. state[1] and sets no bin in either array: no
 *   label or mask value indexes memory unguarded.  K >= C, K <= CAVP_METRICS_MAX_CLASSES, 0 <= ignore < 256.
 * cavp_clipval_combine, per participating frame: the frame is multi-source iff #{v in [0, 256) : hist[n][v] > min_count} >
 *   min_values (the ignore value counts as a value; values >= K are values of their own).  counts[0] (ALL) += conf[n] for every
 *   participating frame, counts[1] (MS) += conf[n] for the multi-source ones (counts: u64 [2][(K+1)*K]); frames[0] / frames[1] +=
 *   the number of frames added to ALL / MS (int64 [2]); state[2] += the count[b] outside [0, T].  flags: u32 [B*T] work array
 *   (overwritten).  Writes hist and conf of the participating frames back to zero.
 * hist and conf must hold at least B*T frames and be ZERO before the first call; combine leaves them zero, so nothing is cleared
 * outside the launches.  state: int64 [4] (device, persistent) {labels >= 256, mask bytes >= K, bad counts, reserved}.  Launch order
 * on one stream: frame_counts, combine.  Integer adds only: the result is independent of arrival order.  No allocation, no
 * synchronisation, no host read of a device value: capturable in a hipGraph. */
int cavp_clipval_frame_counts(const void* pred, int32_t pred_is_mask, const int64_t* labels, const void* count, int32_t count_i64,
                              int32_t B, int32_t T, int32_t C, int64_t HW, int32_t K, int64_t ignore, uint32_t* hist, uint32_t* conf,
                              int64_t* state, void* stream);
int cavp_clipval_combine(uint32_t* hist, uint32_t* conf, uint32_t* flags, const void* count, int32_t count_i64, int32_t B, int32_t T,
                         int32_t K, int32_t min_count, int32_t min_values, uint64_t* counts, int64_t* frames, int64_t* state,
                         void* stream);

/* ---- Video validation (two entry points added to ABI 16; nothing else changed): the per-video J (mask IoU) and F (best F-measure)
 * of the AVSBench object trainer's validation loop (trainer_cavp_avs_obj.py:292-363) for a batch of B videos of T frames at once,
 * restated in tests/_videoval_ref.py ----
 * Frame n = b * T + t takes part iff t < clamp(count[b], 0, T) (count as for clip validation above; NULL: all frames).  A frame
 * that does not take part is not read.  Every pixel of a participating frame has a label v (labels: dense int64 [B*T][HW], never
 * written), a predicted class p and a probability q:
 *   pred_is_mask == 0: pred is dense f32 logits [B*T][C][HW], 2 <= C <= K (any 4-byte aligned base; prob is ignored); p = argmax
 *     over C (first maximal index, a NaN counts as the maximum), q = expf(x[channel] - m) / sum_c expf(x[c] - m), m = max_c x[c]:
 *     the expression, and so the bits, of the F-measure histogram entry point above with C >= 2;
 *   pred_is_mask != 0: pred is a dense u8 class mask [B*T][HW] and prob a dense f32 plane [B*T][HW] (the two outputs of
 *     cavp_seg_predict_nhwc); p = the mask byte, q = the plane's value (C and channel are ignored).
 * 16-byte loads when HW % 4 == 0 and the bases are 16-byte aligned (mask: 4 bytes), element loads otherwise.  With C <= 4 the
 * logits of a pixel are loaded once and held in registers; wider logits are loaded a second time for the softmax.
 *
 * cavp_videoval_frame_stats, per participating frame, all integer adds:
 *   stats[n][4] (int64 scratch) += sum p*v, sum max(p, v), sum (1-v)(1-p), sum v: cavp_mask_iou_stats of (p as int64, labels);
 *   hist[n][2][pr_num+1] (u32 scratch) += the histogram of bin(q) = #{i : thresholds[i] <= q} over all pixels ([n][0]) and over
 *     v != 0 ([n][1]): cavp_fmeasure_hist;
 *   M[(K+1)*K] (u64, global) += the confusion counts of cavp_seg_confusion_nchw (v < 0 or v == ignore: no count; row = v < K ? v : K),
 *     privatised per workgroup in LDS when thresholds, histograms and counts fit 64 KiB together.
 *   state[0] += the labels outside {0, 1, ignore} (they are still counted by the rules above); state[1] += the mask bytes >= K
 *   (counted in stats and hist, no confusion bin): no label or mask value indexes memory unguarded.
 *   thresholds: ascending f32 [pr_num], 1 <= pr_num <= CAVP_VIDEOVAL_MAX_THRESHOLDS.  K <= CAVP_METRICS_MAX_CLASSES.
 * cavp_videoval_combine, one workgroup per video b with c = clamp(count[b], 0, T) > 0 frames, float32, IEEE operations, no
 *   contraction:
 *   J = (sum over t < c ascending of o_t / (u_t + 1e-7)) / c with (o_t, u_t) = (stats[n][0], stats[n][1]), or (stats[n][2], HW)
 *     when stats[n][3] == 0 (mask_iou's empty-target substitution);
 *   per frame and threshold i: tp = sum_{k > i} hist[n][1][k], prec = tp / (sum_{k > i} hist[n][0][k] + 1e-20), recall = tp /
 *     (ysum + 1e-20) with ysum = sum_k hist[n][1][k], f = 1.3 prec recall / (0.3 prec + recall), NaN -> 0; the f of the frames with
 *     ysum > 0 are added in ascending t and divided by the number of those frames (none: 0); F = the maximum over i.
 *   J[slot] and F[slot] (f32 [max_videos]) with slot = state[4] + #{b' < b : clamp(count[b']) > 0}: batch order within a call, call
 *   order across calls; a video with c == 0 takes no slot, one with slot >= max_videos is not stored and counted in state[3].  The
 *   last workgroup to finish (a ticket in state[5], left at 0) adds the number of videos of this call to state[4]: no host read,
 *   the same on every graph replay.  state[2] += the count[b] outside [0, T].  Writes stats and hist of the participating frames
 *   back to zero.
 * stats and hist must hold at least B*T frames and be ZERO before the first call; combine leaves them zero, so nothing is cleared
 * outside the launches.  state: int64 [8] (device, persistent) {labels outside {0, 1, ignore}, mask bytes >= K, bad counts, videos
 * dropped, videos seen, ticket, reserved, reserved}.  Launch order on one stream: frame_stats, combine, with the same count, B, T,
 * HW and pr_num.  B*T <= 65535, HW < 2^31.  The integer results are independent of arrival order, the float tail runs in a fixed
 * order.  No allocation, no synchronisation, no host read of a device value: capturable in a hipGraph. */
#define CAVP_VIDEOVAL_MAX_THRESHOLDS 1024
int cavp_videoval_frame_stats(const void* pred, int32_t pred_is_mask, const float* prob, const int64_t* labels, const void* count,
                              int32_t count_i64, int32_t B, int32_t T, int32_t C, int32_t channel, int64_t HW, int32_t K,
                              int64_t ignore, const float* thresholds, int32_t pr_num, int64_t* stats, uint32_t* hist, uint64_t* M,
                              int64_t* state, void* stream);
int cavp_videoval_combine(int64_t* stats, uint32_t* hist, const void* count, int32_t count_i64, int32_t B, int32_t T, int64_t HW,
                          int32_t pr_num, int32_t max_videos, float* J, float* F, int64_t* state, void* stream);

/* ---- Semantic validation (two entry points added to ABI 16; nothing else changed): the per-frame, per-class IoU and F-score
 * (beta^2 = 0.3) of the AVSBench-semantic metric (utils/avsbench_metrics.py: calc_color_miou_fscore, calc_color_miou,
 * calc_binary_miou) for a batch of B clips of T frames at once, restated in tests/_semval_ref.py ----
 * Frame n = b * T + t takes part iff t < clamp(count[b], 0, T) (count as for clip validation above; NULL: all frames).  A frame
 * that does not take part is not read.  Every pixel of a participating frame has a label v (labels: dense int64 [B*T][HW], never
 * written) and a prediction p: pred_is_mask == 0: pred is dense f32 logits [B*T][K][HW] (C must equal K: the metric takes its
 * class number from the logits; any 4-byte aligned base), p = argmax over K (first maximal index, a NaN counts as the maximum; the
 * reference's softmax in front of it does not change it and is not computed); pred_is_mask != 0: pred is a dense u8 class mask
 * [B*T][HW] (C is ignored).  16-byte loads when HW % 4 == 0 and the bases are aligned (mask: 4 bytes), element loads otherwise.
 *
 * cavp_semval_frame_counts adds, per participating frame, into the per-frame scratch [n][3K + 4] (u32, u32 atomics):
 *   inter[c] = #(p == c and v == c), pred[c] = #(p == c and v >= 0), lab[c] = #(v == c) at [n][c], [n][K + c], [n][2K + c]: the
 *   three torch.histc(bins=K, min=1, max=K) areas of the reference.  A pixel with v < 0 counts in none; one with v >= K (the ignore
 *   value 255 included) counts in pred only, as in the reference, whose histc drops the label.
 *   [n][3K ..]: #(P and G), #(P or G), #(not P and not G), #G over ALL pixels with P = (p != 0), G = (v != 0): calc_binary_miou.
 *   A mask byte p >= K is counted in state[0] and sets none of the class counters (it is foreground in the binary sums): no label
 *   or mask value indexes memory unguarded.  Counters are privatised per workgroup in LDS (3K + 4 words, at most 48 KiB + 16 bytes).
 * cavp_semval_combine, one thread per class c, float32, IEEE operations, no contraction, frames in ascending n:
 *   union = pred + lab - inter, iou = inter / (2.220446049250313e-16f + union), precision = inter / pred, recall = inter / lab,
 *   f = ((1.3f * precision) * recall) / (0.3f * precision + recall) with NaN -> 0, hit = (union != 0).
 *   last[c], last[K + c], last[2K + c] = the sums of iou, f and hit over the call's participating frames, starting from zero (one
 *   call of calc_color_miou_fscore); acc[c], acc[K + c], acc[2K + c] += those sums (the benchmark driver's `miou_pc += _miou_pc`).
 *   Per frame: last[3K + 1 + n] = frame_miou = (sum over c ascending of iou) / #(iou != 0) (NaN when no IoU is non-zero), -1 for a
 *   frame that takes no part; last[3K + 1 + max_frames + n] = the frame's binary IoU = inter / (union + 1e-7f) with (inter, union)
 *   = (#(P and G), #(P or G)), or (#(not P and not G), HW) when #G == 0; -1 likewise.  last[3K] = the sum of the binary IoUs in
 *   ascending n from zero, acc[3K] += it, state[2] += the number of participating frames, state[1] += the count[b] outside [0, T].
 *   acc: f32 [3K + 1], last: f32 [3K + 1 + 2 * max_frames], B*T <= max_frames.  Writes the scratch of the participating frames
 *   back to zero (the last workgroup to finish, by a ticket in state[3] that it leaves at 0).
 * scratch must hold at least B*T frames and be ZERO before the first call; combine leaves it zero, so nothing is cleared outside
 * the launches.  state: int64 [4] (device, persistent) {mask bytes >= K, bad counts, frames, ticket}.  Launch order on one stream:
 * frame_counts, combine, with the same count, B, T, HW and K.  2 <= K <= CAVP_METRICS_MAX_CLASSES, B*T <= 65535, HW < 2^31 (the
 * counts are exact as float32 below 2^24 pixels per frame).  The integer counts are independent of arrival order, the float tail
 * runs in a fixed order.  No allocation, no synchronisation, no host read of a device value: capturable in a hipGraph. */
int cavp_semval_frame_counts(const void* pred, int32_t pred_is_mask, const int64_t* labels, const void* count, int32_t count_i64,
                             int32_t B, int32_t T, int32_t C, int64_t HW, int32_t K, uint32_t* scratch, int64_t* state, void* stream);
int cavp_semval_combine(uint32_t* scratch, const void* count, int32_t count_i64, int32_t B, int32_t T, int64_t HW, int32_t K,
                        int32_t max_frames, float* acc, float* last, int64_t* state, void* stream);

/* ---- Wave stage (two entry points added to ABI 16; nothing else changed): the mono 16 kHz window the reference's data sets cut
 * on the host from a decoded file - Resample(rate, 16000), crop_audio, the sum over the sources resp. the mean over the channels,
 * the one second of a clip (vpo_mono/multi_source/audio/audio_dataset.py:48-70, avss/audio/audio_dataset.py:42-62,
 * avsbench_ms.py:129-134,156-159,169-180, avsbench_s4.py:120-149) - as ONE launch, restated in tests/_wave_ref.py ----
 * raw: [B][S][C][Lmax] float32 (raw_i16 == 0) or int16 (raw_i16 != 0; v stands for v / 32768), contiguous, never written.
 * length, rate_idx, n_ch: int32 [B][S]; select: int32 [B] or NULL.  Per row b, source s with L = length[b][s] > 0, channel c < n_ch:
 *   resample: rate_desc[r] = {o, n, span, stride, tap_off, first_off, shift, fspread} (int32 [n_rates][8], device) with o : n the
 *     reduced ratio rate : 16000; taps + tap_off is the compact float32 filter [n][stride] (the live taps of phase p first, zeros up
 *     to `span`; stride >= span), first + first_off the int32 [n] index of the first live tap of each phase less its minimum,
 *     shift = that minimum less the filter's half width, fspread = the largest entry of first.  L16 = ceil(n * L / o) (64-bit);
 *     y[j] = sum over k < span, ascending, fmaf, of taps[p][k] * xz[(j / n) * o + shift + first[p] + k], p = j % n, xz zero outside
 *     [0, L).  Rate 16000 is {1, 1, 1, 1, ..} with the single tap 1.0f: y = x bit for bit.
 *   crop: mid = L16 / 2, st = mid - sample_len / 2, s0 = st >= 0 ? st : max(L16 + st, 0), s1 = min(st + sample_len, L16),
 *     ln = s1 - s0; w[i] = y[s0 + (ln == sample_len ? i : i % ln)]: crop_audio's slice with its negative-start wrap and repeat.
 *   reduce: m_s[i] = (sum over c ascending of w_{s,c}[i]) / n_ch; out[i] = sum over the present sources ascending of m_s[i].
 *   select != NULL: out holds A_out = sample_len / segments values per row, i = select[b] * A_out + a; else A_out = sample_len.
 * Only the window of y is computed.  out: float32 [B][A_out].
 * Bad input - a length outside [0, Lmax], a rate_idx outside [0, n_rates) or an n_ch outside [1, C] of a present source, a select
 * outside [0, segments), a rate_desc entry that does not fit the three LDS capacities - adds 1 per value to state[0] (int64 [4],
 * device, persistent) and the row is written as zeros; no input value makes the kernel read or write out of bounds.
 * LDS: tab_cap floats for one rate's filter, first_cap int32 for its first-tap indices, x_cap floats for the input span of one
 * tile of cavp_wave_tile() outputs: x_cap >= ((tile - 1) / n + 1) * o + fspread + span for every rate; together at most 160 KiB.
 * Lmax <= 2^28.  No allocation, no synchronisation, no host read of a device value: capturable in a hipGraph. */
int cavp_wave_tile(void);
int cavp_wave_stage(const void* raw, int32_t raw_i16, const int32_t* length, const int32_t* rate_idx, const int32_t* n_ch,
                    const int32_t* select, int32_t B, int32_t S, int32_t C, int64_t Lmax, int32_t sample_len, int32_t segments,
                    const int32_t* rate_desc, int32_t n_rates, const float* taps, const int32_t* first, int32_t tab_cap,
                    int32_t first_cap, int32_t x_cap, int64_t* state, float* out, void* stream);

/* ---- Preview stage (two entry points added to ABI 16; nothing else changed): the three pictures per frame of the reference's
 * Tensorboard.upload_wandb_image (utils/tensor_board.py:90-139) - the de-normalised frame x, the label y and the prediction y_tilde -
 * as bytes on the device, restated in tests/_preview_ref.py.  y and y_tilde are PALETTE INDICES, one byte per pixel; the palette
 * (get_pallete / colorize_mask) is applied on the host ----
 * cavp_preview_panels, B images of HW pixels, every input dense and never written:
 *   x [HW][3] (RGB interleaved), from image f32 [B][3][HW] and mean_std f32 [6] on the device (mean of R, G, B, then std): per
 *     channel v = t * std; v = v + mean; u = v * 255 - three separately rounded float32 operations, never contracted into a fused
 *     multiply-add (DeNormalize's t.mul_(s).add_(m), then ToPILImage's pic.mul(255).byte()); the byte is u truncated toward zero,
 *     taken mod 256 (-1.5 -> 255, 256.7 -> 0, 300 -> 44).  A non-finite u or |u| >= 2^31 writes 0 and adds 1 to state[0] (int64 [4],
 *     device, persistent).  image == NULL (then x == NULL): no x panel.
 *   y [HW], from labels int64 (label_u8 == 0) or uint8 (label_u8 != 0) [B][HW]: the value mod 256 (-1 -> 255, 259 -> 3), numpy's
 *     astype(uint8).  labels == NULL (then y == NULL): no y panel and no propagation below.
 *   y_tilde [HW]: the prediction p, overwritten with 255 where the RAW label equals `ignore` (compared before the wrap: a -1 label
 *     does not propagate).  pred_is_mask == 0: pred is f32 logits [B][C][HW], 1 <= C <= 256, p = argmax over C (first maximal index,
 *     a NaN counts as the maximum: torch.argmax, the rule of the confusion entry points); every logit is read exactly once.
 *     pred_is_mask != 0: pred is a u8 class mask [B][HW] (what cavp_seg_predict_nhwc writes; C is ignored), p = the byte.
 *   Image b's panels start out_stride bytes after image b-1's (out_stride >= the bytes of the present panels).
 *   One thread handles 4 consecutive pixels: 16-byte loads per channel plane and whole-dword stores (three for x, one each for y and
 *   y_tilde) when HW % 4 == 0, out_stride % 4 == 0 and every base is aligned (f32 and int64: 16 bytes, bytes: 4); element accesses
 *   otherwise.  No atomics except the bad counter.
 * cavp_preview_resize: the panels of B images in the dense per-image layout {x [H][W][3] if has_x, y [H][W] if has_y, y_tilde [H][W]}
 *   gathered into the same layout at Ho x Wo: dst(oy, ox) = src(row_tab[oy], col_tab[ox]) (int32 [Ho] / [Wo] on the device, entries
 *   in [0, H) / [0, W): Image.resize(NEAREST)'s source indices, made once on the host).  src and dst do not overlap.
 * No allocation, no synchronisation, no host read of a device value: capturable in a hipGraph. */
int cavp_preview_panels(const float* image, const float* mean_std, const void* labels, int32_t label_u8, const void* pred,
                        int32_t pred_is_mask, int32_t B, int32_t C, int64_t HW, int64_t ignore, uint8_t* x, uint8_t* y,
                        uint8_t* y_tilde, int64_t out_stride, int64_t* state, void* stream);
int cavp_preview_resize(const uint8_t* src, uint8_t* dst, const int32_t* row_tab, const int32_t* col_tab, int32_t B, int32_t H,
                        int32_t W, int32_t Ho, int32_t Wo, int32_t has_x, int32_t has_y, void* stream);

/* ---- Device store (three entry points added to ABI 16; nothing else changed): a frozen, device-resident ragged data set, the
 * sampler of the reference's loaders (RandomSampler / DistributedSampler with drop_last=True, main_vpo_mono.py:188-201) and the
 * gather of one batch into the staging buffers of the frame augmentation and the wave stage, restated in tests/_store_ref.py ----
 * The store: N items packed back to back, no padding, in three byte arenas - frames (item i: [h][w][3] u8 at frame_off[i]), masks
 * ([h][w] u8 at mask_off[i]) and PCM (source s of item i: [n_ch][length] samples of `elem` bytes, 2 = int16 or 4 = float32, at
 * pcm_off[i][s]) - with int64 byte-offset tables frame_off [N], mask_off [N], pcm_off [N][S] and int32 size [N][2] = (h, w),
 * n_src [N], length / rate_idx / n_ch [N][S].  1 <= h <= Hs, 1 <= w <= Ws, 0 <= n_src <= S, 1 <= length <= Lmax, 1 <= n_ch <= Cm.
 * cavp_store_plan, one workgroup: row i < B of step t = state[1] (state: int64 [4], device, persistent, {seed, t, bad_inputs,
 *   reserved}) takes the item index_in[i] when index_in != NULL (an entry outside [0, N) adds 1 to state[2] and becomes 0), else
 *   M = ceil(N / world), spe = M / B (>= 1), e = t / spe, j = (t % spe) * B + i, q = j * world + rank, q -= N if q >= N, item =
 *   pi_e(q): a balanced Feistel network on 2k bits, bits = max(2, bit_length(N - 1)), k = ceil(bits / 2), x = (L << k) | R, 8 rounds
 *   r = 0 .. 7 of (L, R) <- (R, L ^ (f & (2^k - 1))), f = word 0 of Philox4x32-10 at counter (R, r, e_lo, e_hi) under the key
 *   (seed_lo, seed_hi); the whole network is applied again until x < N.  No sort, no stored permutation.
 *   Writes index [B], sizes [B][2], length / n_ch [B][S] (0 for the sources >= n_src), rate_idx [B][S] (present sources only) and
 *   the int64 plan [B][cavp_store_plan_words(S) = 4 + 3 S] = {frame_off, mask_off, h, w, then per source {pcm_off, length, n_ch}},
 *   then state[1] = t + 1 - with or without index_in; the only writer of t.  A table entry that leaves its limits or its arena
 *   (frame_bytes, mask_bytes, pcm_bytes) is counted in state[2] and planned as empty: nothing is read out of bounds.
 * cavp_store_gather, after the plan on the same stream, grid (x, B, 2 + S * Cm): the item's h x w window into out_frames
 *   [B][Hs][Ws][3] and out_masks [B][Hs][Ws] (top-left), channel c < n_ch of source s into out_pcm [B][S][Cm][Lmax] up to length.
 *   Outside the windows, beyond length and in absent channels and sources NOTHING is written.  A row (3w / w / length * elem
 *   bytes; the whole window as one row when w == Ws) is copied as a byte-wise head up to the destination's 16-byte boundary, a
 *   body of 16-byte stores fed by unaligned 16-byte loads, and a byte-wise tail; every access lies inside the row, so no byte
 *   outside an arena is read whatever the last item's alignment.  Work items are (row, 4 KiB chunk) pairs, one wave each.
 * B <= 1024, Hs, Ws <= CAVP_STORE_MAX_STAGE, Lmax <= 2^28, 2 + S * Cm <= 65535, world <= N, ceil(N / world) >= B.
 * No allocation, no synchronisation, no host read of a device value: capturable in a hipGraph. */
#define CAVP_STORE_MAX_STAGE 16384
int cavp_store_plan_words(int32_t S);
int cavp_store_plan(const int64_t* frame_off, const int64_t* mask_off, const int32_t* size, const int32_t* n_src,
                    const int64_t* pcm_off, const int32_t* length, const int32_t* rate_idx, const int32_t* n_ch, int64_t frame_bytes,
                    int64_t mask_bytes, int64_t pcm_bytes, int32_t N, int32_t B, int32_t S, int32_t Hs, int32_t Ws, int32_t Cm,
                    int64_t Lmax, int32_t elem, int32_t rank, int32_t world, const int32_t* index_in, int64_t* state,
                    int32_t* out_index, int32_t* out_sizes, int32_t* out_length, int32_t* out_rate_idx, int32_t* out_n_ch,
                    int64_t* plan, void* stream);
int cavp_store_gather(const uint8_t* frames, const uint8_t* masks, const uint8_t* pcm, const int64_t* plan, int32_t B, int32_t S,
                      int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem, uint8_t* out_frames, uint8_t* out_masks,
                      uint8_t* out_pcm, void* stream);

/* ---- Clip store (four entry points added to ABI 16; nothing else changed): the device store for data sets whose items are clips
 * of up to 32 frames (the reference's S4Dataset / MS3Dataset / AVSS VisualDataset), the frame draw of the clip trainers
 * (trainer_cavp_avs_obj.py:162-172) and the in-order walk of their validation loops, restated in tests/_clips_ref.py ----
 * The store: the three byte arenas of the device store, packed back to back, no padding.  Frame tables over all F frames of all
 * clips: int64 frame_off [F] ([h][w][3] u8 there), int64 mask_off [F] ([h][w] u8 there; -1 = the frame has no mask and takes no
 * byte of the mask arena), int32 size [F][2] = (h, w), 1 <= h <= Hs, 1 <= w <= Ws.  Clip tables over the N clips: int32 first [N]
 * (the clip's frame k is frame first + k of the frame tables), int32 n_frames [N] (1 .. Tmax, Tmax <= 32), uint32 avail [N] (bit k
 * set: a training draw may take frame k; non-zero, no bit >= n_frames, every named frame has a mask), int32 mask_num [N]
 * (0 .. n_frames), int32 tag [N] (the caller's, passed through), and the device store's PCM tables with one row per clip: int32
 * n_src [N], int64 pcm_off [N][S], int32 length / rate_idx / n_ch [N][S].
 * state: int64 [4], device, persistent, {seed, t_train, bad_inputs, t_eval}.  cavp_clips_plan_train reads and writes t_train only,
 *   cavp_clips_plan_eval t_eval only; both add to bad_inputs.
 * cavp_clips_plan_train, one workgroup, one thread per row: row i < B of step t = state[1].
 *   Clip: exactly the item rule of cavp_store_plan (index_in[i], an entry outside [0, N) adds 1 to state[2] and becomes 0; else
 *   pi_e(q) with M, spe, e, j, q as there).
 *   Frame: frame_in[i] when frame_in != NULL; a value that is not a set bit of avail (negative and >= 32 included) adds 1 to
 *   state[2] and becomes the lowest set bit.  Else n = popcount(avail), w = word 0 of Philox4x32-10 at counter (i, 0xC11F, t_lo,
 *   t_hi) under the key (seed_lo, seed_hi) (t with or without index_in; a Feistel counter has c1 < 8, so the two never meet),
 *   r = (uint64(w) * n) >> 32, frame = the position of the r-th (0-based, from bit 0) set bit of avail.
 *   Writes index [B] (the clip), select [B] (the frame), tag [B], sizes [B][2] (the frame's h, w), length / n_ch [B][S] (0 for the
 *   sources >= n_src), rate_idx [B][S] (present sources only), the int64 plan [B][cavp_clips_plan_words(1, S)] and then state[1] =
 *   t + 1.
 * cavp_clips_plan_eval, one workgroup, one thread per (row, frame slot): in order, no shuffle.  M = ceil(N / world), P = ceil(M / B)
 *   steps per pass; step t = state[3] has s = t mod P; row i has q = (s * B + i) * world + rank.  q < N: clip q, index[i] = q,
 *   count[i] = mask_num[q].  q >= N: a padding row - everything below as for clip 0, but index[i] = -1 and count[i] = 0.  Over the P
 *   steps of a pass and all ranks every clip is a non-padding row exactly once.
 *   Writes index, count, n_frames, tag [B], sizes [B * Tmax][2] (slot k < n_frames: the frame's h, w; slot k >= n_frames: the h, w
 *   of the clip's frame 0), length / rate_idx / n_ch as above, the int64 plan [B][cavp_clips_plan_words(Tmax, S)], then state[3] =
 *   t + 1.
 * The plan row: int64 [4 T_out + 3 S] = T_out x {frame_off, mask_off, h, w} (T_out = 1 for train, Tmax for eval; an empty slot has
 *   h = w = 0, a frame without a mask mask_off = -1), then per source {pcm_off, length, n_ch}.
 * Both plans check every table value on the device as cavp_store_plan does: a clip whose first / n_frames / avail leave their
 *   limits, a frame whose size or offsets leave the stage or an arena (train: or that has no mask), a mask_num outside
 *   [0, n_frames] (count becomes 0), a source outside its limits - each adds 1 to state[2] and is planned as empty (sizes 0, 0).
 * cavp_clips_gather, after either plan on the same stream, grid (x, B, 2 T_out + S * Cm): z < T_out the frame of slot z, z < 2 T_out
 *   the mask of slot z - T_out, then channel c of source s at z = 2 T_out + s * Cm + c.  Slot k of row b goes to out_frames
 *   [B][T_out][Hs][Ws][3] and out_masks [B][T_out][Hs][Ws] (top-left h x w window), channel c < n_ch of source s to out_pcm
 *   [B][S][Cm][Lmax] up to length.  An empty slot, the mask of a frame without one, absent channels and sources, and every byte
 *   outside the windows: NOTHING is written.  Rows are copied by the device store's row copy (byte head to the destination's
 *   16-byte boundary, 16-byte stores fed by unaligned 16-byte loads, byte tail, no access outside the row).
 * B <= 1024, B * T_out <= 1024, Tmax <= 32, 2 T_out + S * Cm <= 65535 (beyond: CAVP_ERR_UNSUPPORTED), Hs, Ws <=
 * CAVP_STORE_MAX_STAGE, Lmax <= 2^28, world <= N, and for the train plan ceil(N / world) >= B.
 * No allocation, no synchronisation, no host read of a device value: capturable in a hipGraph. */
#define CAVP_CLIPS_MAX_FRAMES 32
int cavp_clips_plan_words(int32_t T_out, int32_t S);
int cavp_clips_plan_train(const int64_t* frame_off, const int64_t* mask_off, const int32_t* size, const int32_t* first,
                          const int32_t* n_frames, const uint32_t* avail, const int32_t* mask_num, const int32_t* tag,
                          const int32_t* n_src, const int64_t* pcm_off, const int32_t* length, const int32_t* rate_idx,
                          const int32_t* n_ch, int64_t frame_bytes, int64_t mask_bytes, int64_t pcm_bytes, int32_t F, int32_t N,
                          int32_t B, int32_t S, int32_t Tmax, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem,
                          int32_t rank, int32_t world, const int32_t* index_in, const int32_t* frame_in, int64_t* state,
                          int32_t* out_index, int32_t* out_select, int32_t* out_tag, int32_t* out_sizes, int32_t* out_length,
                          int32_t* out_rate_idx, int32_t* out_n_ch, int64_t* plan, void* stream);
int cavp_clips_plan_eval(const int64_t* frame_off, const int64_t* mask_off, const int32_t* size, const int32_t* first,
                         const int32_t* n_frames, const uint32_t* avail, const int32_t* mask_num, const int32_t* tag,
                         const int32_t* n_src, const int64_t* pcm_off, const int32_t* length, const int32_t* rate_idx,
                         const int32_t* n_ch, int64_t frame_bytes, int64_t mask_bytes, int64_t pcm_bytes, int32_t F, int32_t N,
                         int32_t B, int32_t S, int32_t Tmax, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem,
                         int32_t rank, int32_t world, int64_t* state, int32_t* out_index, int32_t* out_count, int32_t* out_n_frames,
                         int32_t* out_tag, int32_t* out_sizes, int32_t* out_length, int32_t* out_rate_idx, int32_t* out_n_ch,
                         int64_t* plan, void* stream);
int cavp_clips_gather(const uint8_t* frames, const uint8_t* masks, const uint8_t* pcm, const int64_t* plan, int32_t B, int32_t T_out,
                      int32_t S, int32_t Hs, int32_t Ws, int32_t Cm, int64_t Lmax, int32_t elem, uint8_t* out_frames,
                      uint8_t* out_masks, uint8_t* out_pcm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CAVP_HIP_H_ */
