// Frame augmentation on the device (include/cavp_hip.h, "frame augmentation"): VisualAugmentation.train_aug of the reference
// (dataset/*/visual/visual_aug.py) on raw uint8 frames and masks - flip, rescale (PIL's two-pass BICUBIC for the frame, its
// NEAREST walk for the mask), ColorJitter, pad, crop, ToTensor + Normalize - as three launches with no host value that depends
// on a device value: plan -> contrast_mean (only with jitter) -> render.  PIL is the specification of every rounding here
// (tests/_augment_ref.py restates it in numpy); the steps that PIL does in double or float are done in the same type and order.
#include "host_util.h"

// the build's -ffp-contract=on would fuse a * b + c: PIL's coefficients, blends and colour conversions are separate roundings
#pragma clang fp contract(off)

constexpr int kAugMaxB = 1024;     // samples of a batch: one thread each in the plan kernel
constexpr int kAugTaps = 12;       // taps of one output index: <= 2 * 2 * (in / out) + 2, in / out <= 2.4 once the output has 6 px
constexpr int kAugTileH = 16, kAugTileW = 64;
constexpr int kAugRows = 64;       // horizontally resampled rows a tile keeps in LDS: <= 15 * (in / out) + 2 * support + 2
constexpr int kAugMaxScales = 16;
constexpr int kAugParams = 16;     // int32 words of a sample's row of the parameter table
// the resize variant's second pass (scaled image -> H x W): in / out <= kRzRatio on either axis
constexpr int kRzRatio = 8;
constexpr int kRzTaps = 34;        // <= 2 * 2 * kRzRatio + 2
constexpr int kRzRows = 154;       // <= 15 * kRzRatio + 2 * 2 * kRzRatio + 2
// the row of the parameter table (cavp_hip.h)
enum { P_FLIP = 0, P_SCALE = 1, P_ORDER = 2, P_BRIGHT = 6, P_CONTRAST = 7, P_SAT = 8, P_HUE = 9, P_TOP = 10, P_LEFT = 11, P_SH = 12,
       P_SW = 13, P_MEAN = 14, P_FLAGS = 15 };

struct AugScales { int n; int num[kAugMaxScales]; };   // scale = num / 64
struct AugNorm { float mean[3], std[3]; int fill[3]; };

// ------------------------------------------------------------------------------------------------------------------- plan
// (aug_u01 - a draw's top 24 bits as a float in [0, 1) - is in common.h, shared with pvt_train.hip's DropPath draw)
__device__ __forceinline__ int aug_below(unsigned r, int n) { return (int)(((unsigned long long)r * (unsigned)n) >> 32); }   // [0, n)

// PIL's NEAREST resize (ImagingScaleAffine): xo = a / 2, xo += a per output index, a = in / out in double; the source index is the
// truncation of the accumulated sum.  tab[j] = source index of output index first + j, -1 past the scaled size (the pad).
__device__ void aug_nearest_walk(int in, int out, int first, int count, bool mirror, int* __restrict__ tab) {
  const double a = (double)in / (double)out;
  double xo = a * 0.5;
  for (int i = 0; i < first; ++i) xo += a;   // the sum has to be walked from index 0: nothing else depends on these steps
  for (int i = first; i < first + count; ++i) {
    int s = -1;
    if (i < out) {
      s = (int)xo;
      s = s < 0 ? 0 : s >= in ? in - 1 : s;
      if (mirror) s = in - 1 - s;
    }
    tab[i - first] = s;
    xo += a;
  }
}

// The resize variant's mask is NEAREST (scaled -> out) of NEAREST (in -> scaled): both walks are monotone, so the first is advanced
// only as far as the second asks and no table of the scaled size exists.  tab[i] = source index of output index i, i in [0, out).
__device__ void aug_nearest_walk2(int in, int scaled, int out, bool mirror, int* __restrict__ tab) {
  const double a1 = (double)in / (double)scaled, a2 = (double)scaled / (double)out;
  double x1 = a1 * 0.5, x2 = a2 * 0.5;
  int at = 0;   // x1 is the accumulated sum of scaled index `at`
  for (int i = 0; i < out; ++i) {
    int s1 = (int)x2;
    s1 = s1 < 0 ? 0 : s1 >= scaled ? scaled - 1 : s1;
    for (; at < s1; ++at) x1 += a1;
    int s = (int)x1;
    s = s < 0 ? 0 : s >= in ? in - 1 : s;
    tab[i] = mirror ? in - 1 - s : s;
    x2 += a2;
  }
}

// resize != 0: the reference's resize_flag variant - streams 0 .. 3 as below, no crop origin (stream 4 is not drawn, top = left = 0,
// words 10, 11 of params_in are ignored), no pad and no crop: nothing is "too small", near_tab is the composed walk to H x W.
__global__ __launch_bounds__(kAugMaxB) void aug_plan_kernel(const int* __restrict__ sizes, int B, int Hs, int Ws, int H, int W,
                                                            AugScales sc, int jitter, int identity, int resize,
                                                            const int* __restrict__ params_in,
                                                            long long* __restrict__ state, int* __restrict__ params,
                                                            int* __restrict__ near_tab, unsigned long long* __restrict__ lsum) {
  __shared__ int s_bad;
  const int t = threadIdx.x;
  const unsigned long long seed = (unsigned long long)state[0], off = (unsigned long long)state[1];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), o0 = (unsigned)off, o1 = (unsigned)(off >> 32);
  if (t == 0) s_bad = 0;
  __syncthreads();   // every thread has read the state before thread 0 moves the offset
  if (t < B) {
    int bad = 0;
    int h = sizes[2 * t], w = sizes[2 * t + 1];
    if (h < 1 || h > Hs || w < 1 || w > Ws) {
      bad = 1;
      h = h < 1 ? 1 : h > Hs ? Hs : h;
      w = w < 1 ? 1 : w > Ws ? Ws : w;
    }
    int flip = 0, si = 0, ord[4] = {0, 1, 2, 3}, hue = 0, top = 0, left = 0;
    float fb = 1.0f, fc = 1.0f, fs = 1.0f;
    unsigned long long k4 = 0ull;
    if (identity) {            // the test-time path: scale 1 is entry `identity - 1` of a one-entry list
    } else if (params_in) {
      const int* p = params_in + (size_t)t * kAugParams;
      flip = p[P_FLIP]; si = p[P_SCALE]; hue = p[P_HUE]; top = p[P_TOP]; left = p[P_LEFT];
      if ((unsigned)flip > 1u) { bad = 1; flip = 0; }
      if (si < 0 || si >= sc.n) { bad = 1; si = 0; }
      if (jitter) {
        int seen = 0;
        for (int k = 0; k < 4; ++k) {
          ord[k] = p[P_ORDER + k];
          if ((unsigned)ord[k] < 4u) seen |= 1 << ord[k];
        }
        fb = __int_as_float(p[P_BRIGHT]); fc = __int_as_float(p[P_CONTRAST]); fs = __int_as_float(p[P_SAT]);
        // (a NaN fails every comparison)
        if (seen != 15 || (unsigned)hue > 255u || !(fb >= 0.0f && fb <= 16.0f) || !(fc >= 0.0f && fc <= 16.0f) || !(fs >= 0.0f && fs <= 16.0f)) {
          bad = 1;
          ord[0] = 0; ord[1] = 1; ord[2] = 2; ord[3] = 3;
          hue = 0; fb = fc = fs = 1.0f;
        }
      }
    } else {
      // Philox4x32-10, counter = (sample, stream, offset_lo, offset_hi), key = seed: the device sampler's convention
      const unsigned long long d0 = philox_key((unsigned)t, 0u, o0, o1, k0, k1);
      flip = aug_u01((unsigned)(d0 >> 32)) > 0.5f ? 1 : 0;
      si = aug_below((unsigned)d0, sc.n);
      if (jitter) {
        const unsigned long long d1 = philox_key((unsigned)t, 1u, o0, o1, k0, k1), d2 = philox_key((unsigned)t, 2u, o0, o1, k0, k1),
                                 d3 = philox_key((unsigned)t, 3u, o0, o1, k0, k1);
        int code = aug_below((unsigned)(d1 >> 32), 24);   // the code-th permutation of 0..3 in lexicographic order
        int pool[4] = {0, 1, 2, 3};
        for (int k = 0, f = 6; k < 4; ++k) {
          const int j = code / f;
          code -= j * f;
          ord[k] = pool[j];
          for (int m = j; m < 3; ++m) pool[m] = pool[m + 1];
          if (k < 3) f /= (3 - k);
        }
        fb = 0.5f + aug_u01((unsigned)d1);
        fc = 0.5f + aug_u01((unsigned)(d2 >> 32));
        fs = 0.5f + aug_u01((unsigned)d2);
        const float hf = -0.25f + 0.5f * aug_u01((unsigned)(d3 >> 32));
        hue = ((int)(hf * 255.0f)) & 255;                 // torchvision: uint8(hue * 255), truncated, mod 256
      }
      if (!resize) k4 = philox_key((unsigned)t, 4u, o0, o1, k0, k1);
    }
    if (resize) top = left = 0;
    // scaled size: int(h * s) with s = num / 64 is the exact integer floor(h * num / 64)
    const int num = identity ? 64 : sc.num[si];
    int sh = (int)(((long long)h * num) >> 6), sw = (int)(((long long)w * num) >> 6);
    if (sh < 1 || sw < 1) {    // PIL refuses an empty image
      bad = 1;
      sh = sh < 1 ? 1 : sh;
      sw = sw < 1 ? 1 : sw;
    }
    // the reference's pad, literally: tgt_h against the width, tgt_w against the height
    int ph = sh, pw = sw;
    if (!identity && min(sh, sw) < min(H, W)) {
      pw = sw + max(H - sw, 0);
      ph = sh + max(W - sh, 0);
    }
    if (identity) { ph = max(sh, H); pw = max(sw, W); }   // eval_: the top-left window, fill where the frame is smaller
    if (resize) { ph = H; pw = W; }                      // no pad, no crop: the origin is (0, 0) by construction
    if (ph < H || pw < W) bad = 1;                       // RandomCrop.get_params raises here
    const int tmax = max(ph - H, 0), lmax = max(pw - W, 0);
    if (resize) {
    } else if (!identity && !params_in) {
      top = aug_below((unsigned)(k4 >> 32), tmax + 1);
      left = aug_below((unsigned)k4, lmax + 1);
    } else if (top < 0 || top > tmax || left < 0 || left > lmax) {
      bad = 1;
      top = top < 0 ? 0 : top > tmax ? tmax : top;
      left = left < 0 ? 0 : left > lmax ? lmax : left;
    }
    int* q = params + (size_t)t * kAugParams;
    q[P_FLIP] = flip; q[P_SCALE] = si;
    for (int k = 0; k < 4; ++k) q[P_ORDER + k] = ord[k];
    q[P_BRIGHT] = __float_as_int(fb); q[P_CONTRAST] = __float_as_int(fc); q[P_SAT] = __float_as_int(fs);
    q[P_HUE] = hue; q[P_TOP] = top; q[P_LEFT] = left; q[P_SH] = sh; q[P_SW] = sw; q[P_MEAN] = -1; q[P_FLAGS] = bad;
    lsum[t] = 0ull;
    int* tab = near_tab + (size_t)t * (H + W);
    if (resize) {
      aug_nearest_walk2(h, sh, H, false, tab);
      aug_nearest_walk2(w, sw, W, flip != 0, tab + H);
    } else {
      aug_nearest_walk(h, sh, top, H, false, tab);
      aug_nearest_walk(w, sw, left, W, flip != 0, tab + H);
    }
    if (bad) atomicAdd(&s_bad, 1);
  }
  __syncthreads();
  if (t == 0) {
    state[1] = (long long)(off + 1ull);
    state[2] += s_bad;
  }
}

// ------------------------------------------------------------------------------------------------------ resize of one tile
__device__ __forceinline__ double aug_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// PIL's precompute_coeffs + normalize_coeffs_8bpc for output index i of an in -> out BICUBIC pass: first tap, tap count and
// the taps at 22 fractional bits.  in == out gives the identity (one tap of 1 << 22).  TAPS: the capacity of k (kAugTaps for the
// scale pass, kRzTaps for the resize variant's second pass).
template <int TAPS>
__device__ void aug_coeffs(int in, int out, int i, int* __restrict__ first, int* __restrict__ count, int* __restrict__ k) {
  const double scale = (double)in / (double)out;
  const double fscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fscale, ss = 1.0 / fscale;
  const double center = (i + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  int n = xmax - xmin;
  if (n > TAPS) n = TAPS;
  double w[TAPS], ww = 0.0;
#pragma unroll
  for (int x = 0; x < TAPS; ++x) {
    w[x] = x < n ? aug_bicubic((x + xmin - center + 0.5) * ss) : 0.0;
    if (x < n) ww += w[x];
  }
#pragma unroll
  for (int x = 0; x < TAPS; ++x) {
    double v = w[x];
    if (ww != 0.0) v = v / ww;
    v = v * 4194304.0;
    k[x] = x < n ? (v < 0.0 ? (int)(-0.5 + v) : (int)(0.5 + v)) : 0;
  }
  *first = xmin;
  *count = n;
}

__device__ __forceinline__ int aug_clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

struct AugTileLds {
  int hk[kAugTileW][kAugTaps + 1];   // (+1: the stride is odd, the columns of a wave fall into different banks)
  int vk[kAugTileH][kAugTaps + 1];
  int hmin[kAugTileW], hn[kAugTileW], vmin[kAugTileH], vn[kAugTileH];
  unsigned rows[kAugRows][kAugTileW];   // the horizontal pass, rounded and clipped to uint8: r | g << 8 | b << 16
};

// The 16 x 64 tile at (y0, x0) of the sh x sw BICUBIC resize of the (mirrored if flip) h x w frame in a slot with row pitch
// `pitch` bytes.  Thread t owns column t & 63, rows (t >> 6) + 4 j; px[j] = r | g << 8 | b << 16, valid where the pixel lies
// inside the scaled image (bit j of the result).  256 threads, every one must call.
__device__ unsigned aug_resize_tile(const unsigned char* __restrict__ frame, int pitch, int h, int w, int sh, int sw, int flip, int y0,
                                    int x0, AugTileLds& L, unsigned px[4]) {
  const int t = threadIdx.x;
  __syncthreads();   // the previous use of L is over
  if (t < kAugTileW) {
    const int x = x0 + t;
    int first = 0, count = 0;
    if (x < sw) aug_coeffs<kAugTaps>(w, sw, x, &first, &count, L.hk[t]);
    L.hmin[t] = first;
    L.hn[t] = count;
  } else if (t < kAugTileW + kAugTileH) {
    const int r = t - kAugTileW, y = y0 + r;
    int first = 0, count = 0;
    if (y < sh) aug_coeffs<kAugTaps>(h, sh, y, &first, &count, L.vk[r]);
    L.vmin[r] = first;
    L.vn[r] = count;
  }
  __syncthreads();
  const int ylast = min(kAugTileH - 1, sh - 1 - y0);
  unsigned valid = 0u;
  if (ylast < 0 || x0 >= sw) return valid;   // (uniform over the workgroup)
  const int r0 = L.vmin[0];
  int nrows = L.vmin[ylast] + L.vn[ylast] - r0;
  nrows = nrows > kAugRows ? kAugRows : nrows;
  for (int idx = t; idx < nrows * kAugTileW; idx += 256) {
    const int rr = idx >> 6, x = idx & 63;
    unsigned v = 0u;
    if (x0 + x < sw) {
      const int sy = min(r0 + rr, h - 1);
      const unsigned char* row = frame + (size_t)sy * pitch;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      const int first = L.hmin[x], n = L.hn[x];
      for (int k = 0; k < n; ++k) {
        int sx = min(first + k, w - 1);
        if (flip) sx = w - 1 - sx;
        const unsigned char* p = row + 3 * sx;
        const int c = L.hk[x][k];
        a0 += p[0] * c;
        a1 += p[1] * c;
        a2 += p[2] * c;
      }
      v = (unsigned)aug_clip8(a0) | ((unsigned)aug_clip8(a1) << 8) | ((unsigned)aug_clip8(a2) << 16);
    }
    L.rows[rr][x] = v;
  }
  __syncthreads();
  const int x = t & 63;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = (t >> 6) + 4 * j;
    px[j] = 0u;
    if (y <= ylast && x0 + x < sw) {
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      const int first = L.vmin[y] - r0, n = L.vn[y];
      for (int k = 0; k < n; ++k) {
        const unsigned v = L.rows[min(first + k, kAugRows - 1)][x];
        const int c = L.vk[y][k];
        a0 += (int)(v & 255u) * c;
        a1 += (int)((v >> 8) & 255u) * c;
        a2 += (int)((v >> 16) & 255u) * c;
      }
      px[j] = (unsigned)aug_clip8(a0) | ((unsigned)aug_clip8(a1) << 8) | ((unsigned)aug_clip8(a2) << 16);
      valid |= 1u << j;
    }
  }
  return valid;
}

// ------------------------------------------------------------------------------------------------------------- ColorJitter
__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) of one byte: f is a C float; inside [0, 1] the float result is truncated, outside clamped first
__device__ __forceinline__ int aug_blend(int deg, int v, float f) {
  if (f == 0.0f) return deg;
  if (f == 1.0f) return v;
  const float tmp = (float)deg + f * (float)(v - deg);
  if (f >= 0.0f && f <= 1.0f) return (int)tmp & 255;
  return tmp <= 0.0f ? 0 : tmp >= 255.0f ? 255 : (int)tmp;
}

// a / b of two small integers as the correctly rounded float (the double quotient is never near a float's rounding boundary)
__device__ __forceinline__ float aug_divf(int a, int b) { return (float)((double)a / (double)b); }

// PIL's rgb2hsv, H += shift mod 256, PIL's hsv2rgb: both lossy, float and double steps as in Convert.c
__device__ void aug_hue(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const int cr = maxc - minc;
    const float s = aug_divf(cr, maxc);
    const float rc = aug_divf(maxc - r, cr), gc = aug_divf(maxc - g, cr), bc = aug_divf(maxc - b, cr);
    float hf;
    if (r == maxc)
      hf = bc - gc;
    else if (g == maxc)
      hf = (float)(2.0 + (double)rc - (double)bc);
    else
      hf = (float)(4.0 + (double)gc - (double)rc);
    const double hd = (double)hf / 6.0 + 1.0;
    hf = (float)(hd - floor(hd));          // fmod(hd, 1.0), exact for hd in [0.8, 1.9)
    uh = (int)((double)hf * 255.0);
    us = (int)((double)s * 255.0);
    uh = uh < 0 ? 0 : uh > 255 ? 255 : uh;
    us = us < 0 ? 0 : us > 255 ? 255 : us;
  }
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = uv;
    return;
  }
  const double h6 = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const double f = (double)(float)(h6 - (double)i);
  const double fs = (double)(float)((double)(float)us / 255.0);
  const double v = (double)uv;
  int p = (int)round(v * (1.0 - fs)), q = (int)round(v * (1.0 - fs * f)), tt = (int)round(v * (1.0 - fs * (1.0 - f)));
  p = p < 0 ? 0 : p > 255 ? 255 : p;
  q = q < 0 ? 0 : q > 255 ? 255 : q;
  tt = tt < 0 ? 0 : tt > 255 ? 255 : tt;
  switch (i % 6) {
    case 0: r = uv; g = tt; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = tt; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = tt; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
  }
}

struct AugJitter { int ord[4]; float b, c, s; int hue; };

__device__ __forceinline__ AugJitter aug_load_jitter(const int* __restrict__ p) {
  AugJitter j;
  for (int k = 0; k < 4; ++k) j.ord[k] = p[P_ORDER + k];
  j.b = __int_as_float(p[P_BRIGHT]); j.c = __int_as_float(p[P_CONTRAST]); j.s = __int_as_float(p[P_SAT]);
  j.hue = p[P_HUE];
  return j;
}

// the four operations in the sample's order; mean < 0: stop in front of the contrast operation (the pass that finds the mean)
__device__ unsigned aug_jitter_pixel(unsigned px, const AugJitter& j, int mean) {
  int r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u;
  for (int k = 0; k < 4; ++k) {
    const int op = j.ord[k];
    if (op == 0) {
      r = aug_blend(0, r, j.b); g = aug_blend(0, g, j.b); b = aug_blend(0, b, j.b);
    } else if (op == 1) {
      if (mean < 0) break;
      r = aug_blend(mean, r, j.c); g = aug_blend(mean, g, j.c); b = aug_blend(mean, b, j.c);
    } else if (op == 2) {
      const int l = aug_luma(r, g, b);
      r = aug_blend(l, r, j.s); g = aug_blend(l, g, j.s); b = aug_blend(l, b, j.s);
    } else {
      aug_hue(r, g, b, j.hue);
    }
  }
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// ---------------------------------------------------------------------------------------------------------- contrast mean
// Sum of L over the WHOLE scaled image after the operations in front of the contrast one: exact integers, one 64-bit atomic per
// workgroup - the order of the additions cannot change the sum.  grid = (tiles of the largest scaled width, of the height, B).
__global__ __launch_bounds__(256) void aug_contrast_mean_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ sizes,
                                                                int Hs, int Ws, const int* __restrict__ params,
                                                                unsigned long long* __restrict__ lsum) {
  __shared__ AugTileLds L;
  __shared__ unsigned s_sum;
  const int b = blockIdx.z;
  const int* p = params + (size_t)b * kAugParams;
  const int sh = p[P_SH], sw = p[P_SW];
  const int y0 = blockIdx.y * kAugTileH, x0 = blockIdx.x * kAugTileW;
  if (y0 >= sh || x0 >= sw) return;
  const int h = min(max(sizes[2 * b], 1), Hs), w = min(max(sizes[2 * b + 1], 1), Ws);
  if (threadIdx.x == 0) s_sum = 0u;
  unsigned px[4];
  const unsigned valid = aug_resize_tile(frames + (size_t)b * Hs * Ws * 3, Ws * 3, h, w, sh, sw, p[P_FLIP], y0, x0, L, px);
  const AugJitter j = aug_load_jitter(p);
  unsigned mine = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (valid & (1u << k)) {
      const unsigned v = aug_jitter_pixel(px[k], j, -1);
      mine += (unsigned)aug_luma(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u);
    }
  atomicAdd(&s_sum, mine);   // <= 1024 * 255: no overflow
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&lsum[b], (unsigned long long)s_sum);
}

// ------------------------------------------------------------------------------------------------------------------ render
// One 16 x 64 tile of the crop window per workgroup: resize tile at (top, left) + the tile's origin, jitter, pad fill, /255,
// normalise, NCHW store; the mask through the plan kernel's nearest tables.  grid = (ceil(W / 64), ceil(H / 16), B).
__global__ __launch_bounds__(256) void aug_render_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ masks,
                                                         const int* __restrict__ sizes, int Hs, int Ws, int H, int W, AugNorm nm,
                                                         int jitter, int* __restrict__ params, const int* __restrict__ near_tab,
                                                         const unsigned long long* __restrict__ lsum, float* __restrict__ image,
                                                         long long* __restrict__ label) {
  __shared__ AugTileLds L;
  const int b = blockIdx.z, t = threadIdx.x;
  int* p = params + (size_t)b * kAugParams;
  const int sh = p[P_SH], sw = p[P_SW], top = p[P_TOP], left = p[P_LEFT];
  const int oy0 = blockIdx.y * kAugTileH, ox0 = blockIdx.x * kAugTileW;
  const int h = min(max(sizes[2 * b], 1), Hs), w = min(max(sizes[2 * b + 1], 1), Ws);
  int mean = 0;
  if (jitter) {   // ImageEnhance.Contrast: int(sum / n + 0.5) as the exact integer floor((2 sum + n) / 2n)
    const unsigned long long n = (unsigned long long)sh * (unsigned long long)sw;
    mean = (int)((2ull * lsum[b] + n) / (2ull * n));
    mean = mean > 255 ? 255 : mean;
    if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) p[P_MEAN] = mean;
  }
  unsigned px[4];
  const unsigned valid = aug_resize_tile(frames + (size_t)b * Hs * Ws * 3, Ws * 3, h, w, sh, sw, p[P_FLIP], top + oy0, left + ox0, L, px);
  AugJitter j;
  if (jitter) j = aug_load_jitter(p);
  const int x = t & 63, ox = ox0 + x;
  if (ox >= W) return;
  const int* ytab = near_tab + (size_t)b * (H + W);
  const int sx = ytab[H + ox];
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int oy = oy0 + (t >> 6) + 4 * k;
    if (oy >= H) continue;
    unsigned v = (unsigned)nm.fill[0] | ((unsigned)nm.fill[1] << 8) | ((unsigned)nm.fill[2] << 16);
    if (valid & (1u << k)) v = jitter ? aug_jitter_pixel(px[k], j, mean) : px[k];
    float* o = image + (size_t)b * 3 * plane + (size_t)oy * W + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)((v >> (8 * c)) & 255u) / 255.0f;   // ToTensor
      o[c * plane] = (u - nm.mean[c]) / nm.std[c];               // Normalize
    }
    const int sy = ytab[oy];
    long long m = 255;
    if (sy >= 0 && sx >= 0) m = (long long)masks[(size_t)b * Hs * Ws + (size_t)sy * Ws + sx];
    label[(size_t)b * plane + (size_t)oy * W + ox] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------- resize variant
// The reference's resize_flag = True (dataset/avss/visual/visual_aug.py): flip, random scale, jitter, then a second BICUBIC /
// NEAREST resize to H x W in place of pad + crop.  PIL rounds to uint8 between the two resizes and the contrast mean is over
// the whole scaled image, so the scaled, flipped, jittered image is stored once (4 bytes per pixel) and resampled from there.

// scratch [B][mh][mw] (r | g << 8 | b << 16): the tile at (16 blockIdx.y, 64 blockIdx.x) of sample blockIdx.z's scaled image
__global__ __launch_bounds__(256) void aug_resize_store_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ sizes,
                                                               int Hs, int Ws, int mh, int mw, int jitter, int* __restrict__ params,
                                                               const unsigned long long* __restrict__ lsum,
                                                               unsigned* __restrict__ scratch) {
  __shared__ AugTileLds L;
  const int b = blockIdx.z, t = threadIdx.x;
  int* p = params + (size_t)b * kAugParams;
  const int sh = min(p[P_SH], mh), sw = min(p[P_SW], mw);
  const int y0 = blockIdx.y * kAugTileH, x0 = blockIdx.x * kAugTileW;
  if (y0 >= sh || x0 >= sw) return;
  const int h = min(max(sizes[2 * b], 1), Hs), w = min(max(sizes[2 * b + 1], 1), Ws);
  int mean = 0;
  if (jitter) {   // as in the render kernel of the crop variant
    const unsigned long long n = (unsigned long long)p[P_SH] * (unsigned long long)p[P_SW];
    mean = (int)((2ull * lsum[b] + n) / (2ull * n));
    mean = mean > 255 ? 255 : mean;
    if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) p[P_MEAN] = mean;
  }
  unsigned px[4];
  const unsigned valid = aug_resize_tile(frames + (size_t)b * Hs * Ws * 3, Ws * 3, h, w, sh, sw, p[P_FLIP], y0, x0, L, px);
  AugJitter j;
  if (jitter) j = aug_load_jitter(p);
  const int x = x0 + (t & 63);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + (t >> 6) + 4 * k;
    if (valid & (1u << k)) scratch[((size_t)b * mh + y) * mw + x] = jitter ? aug_jitter_pixel(px[k], j, mean) : px[k];
  }
}

struct AugResizeLds {
  int hk[kAugTileW][kRzTaps + 1];   // (odd stride, as in AugTileLds)
  int vk[kAugTileH][kRzTaps + 1];
  int hmin[kAugTileW], hn[kAugTileW], vmin[kAugTileH], vn[kAugTileH];
  unsigned rows[kRzRows][kAugTileW];
};

// One 16 x 64 tile of the H x W output per workgroup: two-pass BICUBIC from a source of per-sample size (ih, iw) - the scratch
// of the store pass (SRC3 = false, 4 bytes per pixel) or, for eval_, the staged frame itself (SRC3 = true, 3 bytes per pixel) -
// then /255, normalise, NCHW store; the mask through the plan kernel's composed nearest table.
template <bool SRC3>
__global__ __launch_bounds__(256) void aug_resize_render_kernel(const unsigned char* __restrict__ src, long long sample_bytes,
                                                                int pitch_bytes, int cap_h, int cap_w,
                                                                const unsigned char* __restrict__ masks, const int* __restrict__ sizes,
                                                                int Hs, int Ws, int H, int W, AugNorm nm, const int* __restrict__ params,
                                                                const int* __restrict__ near_tab, float* __restrict__ image,
                                                                long long* __restrict__ label) {
  __shared__ AugResizeLds L;
  const int b = blockIdx.z, t = threadIdx.x;
  const int* p = params + (size_t)b * kAugParams;
  // the source's size: never beyond what the buffer holds
  const int ih = SRC3 ? min(max(sizes[2 * b], 1), Hs) : min(max(p[P_SH], 1), cap_h);
  const int iw = SRC3 ? min(max(sizes[2 * b + 1], 1), Ws) : min(max(p[P_SW], 1), cap_w);
  const int y0 = blockIdx.y * kAugTileH, x0 = blockIdx.x * kAugTileW;
  const unsigned char* img = src + (size_t)b * sample_bytes;
  if (t < kAugTileW) {
    int first = 0, count = 0;
    if (x0 + t < W) aug_coeffs<kRzTaps>(iw, W, x0 + t, &first, &count, L.hk[t]);
    L.hmin[t] = first;
    L.hn[t] = count;
  } else if (t < kAugTileW + kAugTileH) {
    const int r = t - kAugTileW;
    int first = 0, count = 0;
    if (y0 + r < H) aug_coeffs<kRzTaps>(ih, H, y0 + r, &first, &count, L.vk[r]);
    L.vmin[r] = first;
    L.vn[r] = count;
  }
  __syncthreads();
  const int ylast = min(kAugTileH - 1, H - 1 - y0);   // >= 0: the grid covers H
  const int r0 = L.vmin[0];
  int nrows = L.vmin[ylast] + L.vn[ylast] - r0;
  nrows = nrows > kRzRows ? kRzRows : nrows;
  for (int idx = t; idx < nrows * kAugTileW; idx += 256) {
    const int rr = idx >> 6, x = idx & 63;
    unsigned v = 0u;
    if (x0 + x < W) {
      const unsigned char* row = img + (size_t)min(r0 + rr, ih - 1) * pitch_bytes;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      const int first = L.hmin[x], n = L.hn[x];
      for (int k = 0; k < n; ++k) {
        const int sx = min(first + k, iw - 1);
        const int c = L.hk[x][k];
        if (SRC3) {
          const unsigned char* q = row + 3 * sx;
          a0 += q[0] * c;
          a1 += q[1] * c;
          a2 += q[2] * c;
        } else {
          const unsigned q = ((const unsigned*)row)[sx];
          a0 += (int)(q & 255u) * c;
          a1 += (int)((q >> 8) & 255u) * c;
          a2 += (int)((q >> 16) & 255u) * c;
        }
      }
      v = (unsigned)aug_clip8(a0) | ((unsigned)aug_clip8(a1) << 8) | ((unsigned)aug_clip8(a2) << 16);
    }
    L.rows[rr][x] = v;
  }
  __syncthreads();
  const int x = t & 63, ox = x0 + x;
  if (ox >= W) return;
  const int* ytab = near_tab + (size_t)b * (H + W);
  const int sx = ytab[H + ox];
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = (t >> 6) + 4 * j, oy = y0 + y;
    if (y > ylast) continue;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    const int first = L.vmin[y] - r0, n = L.vn[y];
    for (int k = 0; k < n; ++k) {
      const unsigned v = L.rows[min(first + k, kRzRows - 1)][x];
      const int c = L.vk[y][k];
      a0 += (int)(v & 255u) * c;
      a1 += (int)((v >> 8) & 255u) * c;
      a2 += (int)((v >> 16) & 255u) * c;
    }
    const int px[3] = {aug_clip8(a0), aug_clip8(a1), aug_clip8(a2)};
    float* o = image + (size_t)b * 3 * plane + (size_t)oy * W + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)px[c] / 255.0f;               // ToTensor
      o[c * plane] = (u - nm.mean[c]) / nm.std[c];         // Normalize
    }
    const int sy = ytab[oy];
    long long m = 255;
    if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) m = (long long)masks[(size_t)b * Hs * Ws + (size_t)sy * Ws + sx];
    label[(size_t)b * plane + (size_t)oy * W + ox] = m;
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static bool aug_shape_ok(int B, int Hs, int Ws, int H, int W) {
  return B >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1;
}
static bool aug_shape_supported(int B, int Hs, int Ws, int H, int W) {
  return B <= kAugMaxB && Hs <= 16384 && Ws <= 16384 && H <= Hs && W <= Ws;
}

// the resize variant: the output may be larger than the slot (an upscale), but the second pass holds at most kRzTaps taps, so the
// largest scaled side may be at most kRzRatio times the output side
static bool aug_resize_supported(int B, int Hs, int Ws, int H, int W, int max_scale64) {
  if (B > kAugMaxB || Hs > 16384 || Ws > 16384 || H > 16384 || W > 16384 || max_scale64 < 32 || max_scale64 > 256) return false;
  const long long mh = ((long long)Hs * max_scale64) >> 6, mw = ((long long)Ws * max_scale64) >> 6;
  return mh <= (long long)kRzRatio * H && mw <= (long long)kRzRatio * W;
}

static int aug_plan_launch(const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* scales64,
                           int32_t n_scales, int32_t jitter, int32_t identity, int resize, const int32_t* params_in, int64_t* state,
                           int32_t* params, int32_t* near_tab, uint64_t* lsum, void* stream) {
  if (!sizes || !state || !params || !near_tab || !lsum || !aug_shape_ok(B, Hs, Ws, H, W)) return CAVP_ERR_BAD_ARG;
  if (!identity && (!scales64 || n_scales < 1)) return CAVP_ERR_BAD_ARG;
  if (n_scales > kAugMaxScales) return CAVP_ERR_UNSUPPORTED;
  if (resize) {
    int mx = identity ? 64 : 0;
    for (int i = 0; !identity && i < n_scales; ++i) mx = scales64[i] > mx ? scales64[i] : mx;
    if (!aug_resize_supported(B, Hs, Ws, H, W, mx > 256 ? 256 : mx)) return CAVP_ERR_UNSUPPORTED;
  } else if (!aug_shape_supported(B, Hs, Ws, H, W)) {
    return CAVP_ERR_UNSUPPORTED;
  }
  AugScales sc;
  sc.n = identity ? 1 : n_scales;
  for (int i = 0; i < kAugMaxScales; ++i) sc.num[i] = 64;
  for (int i = 0; !identity && i < n_scales; ++i) {
    if (scales64[i] < 32 || scales64[i] > 256) return CAVP_ERR_UNSUPPORTED;   // 0.5 .. 4: the tap and LDS row bounds above
    sc.num[i] = scales64[i];
  }
  aug_plan_kernel<<<1, kAugMaxB, 0, (hipStream_t)stream>>>(sizes, B, Hs, Ws, H, W, sc, jitter ? 1 : 0, identity ? 1 : 0, resize, params_in,
                                                           (long long*)state, params, near_tab, (unsigned long long*)lsum);
  CHECK_LAUNCH();
}

extern "C" int cavp_aug_plan(const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* scales64,
                             int32_t n_scales, int32_t jitter, int32_t identity, const int32_t* params_in, int64_t* state,
                             int32_t* params, int32_t* near_tab, uint64_t* lsum, void* stream) {
  return aug_plan_launch(sizes, B, Hs, Ws, H, W, scales64, n_scales, jitter, identity, 0, params_in, state, params, near_tab, lsum, stream);
}

extern "C" int cavp_aug_plan_resize(const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                                    const int32_t* scales64, int32_t n_scales, int32_t jitter, int32_t identity,
                                    const int32_t* params_in, int64_t* state, int32_t* params, int32_t* near_tab, uint64_t* lsum,
                                    void* stream) {
  return aug_plan_launch(sizes, B, Hs, Ws, H, W, scales64, n_scales, jitter, identity, 1, params_in, state, params, near_tab, lsum, stream);
}

extern "C" int cavp_aug_contrast_mean(const uint8_t* frames, const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws,
                                      int32_t max_scale64, const int32_t* params, uint64_t* lsum, void* stream) {
  if (!frames || !sizes || !params || !lsum || B < 1 || Hs < 1 || Ws < 1) return CAVP_ERR_BAD_ARG;
  if (B > kAugMaxB || Hs > 16384 || Ws > 16384 || max_scale64 < 32 || max_scale64 > 256) return CAVP_ERR_UNSUPPORTED;
  const int mh = (int)(((long long)Hs * max_scale64) >> 6), mw = (int)(((long long)Ws * max_scale64) >> 6);
  const dim3 grid((mw + kAugTileW - 1) / kAugTileW, (mh + kAugTileH - 1) / kAugTileH, B);
  if (grid.y > 65535u) return CAVP_ERR_UNSUPPORTED;
  aug_contrast_mean_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(frames, sizes, Hs, Ws, params, (unsigned long long*)lsum);
  CHECK_LAUNCH();
}

extern "C" int cavp_aug_render(const uint8_t* frames, const uint8_t* masks, const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws,
                               int32_t H, int32_t W, const float* mean3, const float* std3, const int32_t* fill3, int32_t jitter,
                               int32_t* params, const int32_t* near_tab, const uint64_t* lsum, float* image, int64_t* label,
                               void* stream) {
  if (!frames || !masks || !sizes || !mean3 || !std3 || !fill3 || !params || !near_tab || !lsum || !image || !label ||
      !aug_shape_ok(B, Hs, Ws, H, W))
    return CAVP_ERR_BAD_ARG;
  if (!aug_shape_supported(B, Hs, Ws, H, W)) return CAVP_ERR_UNSUPPORTED;
  AugNorm nm;
  for (int c = 0; c < 3; ++c) {   // mean3 / std3 / fill3 are HOST arrays: constants of the augmentation, passed by value
    if (!(std3[c] > 0.0f) || fill3[c] < 0 || fill3[c] > 255) return CAVP_ERR_BAD_ARG;
    nm.mean[c] = mean3[c];
    nm.std[c] = std3[c];
    nm.fill[c] = fill3[c];
  }
  const dim3 grid((W + kAugTileW - 1) / kAugTileW, (H + kAugTileH - 1) / kAugTileH, B);
  aug_render_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(frames, masks, sizes, Hs, Ws, H, W, nm, jitter ? 1 : 0, params, near_tab,
                                                           (const unsigned long long*)lsum, image, (long long*)label);
  CHECK_LAUNCH();
}

extern "C" int cavp_aug_resize_store(const uint8_t* frames, const int32_t* sizes, int32_t B, int32_t Hs, int32_t Ws, int32_t max_scale64,
                                     int32_t jitter, int32_t* params, const uint64_t* lsum, uint32_t* scratch, void* stream) {
  if (!frames || !sizes || !params || !lsum || !scratch || B < 1 || Hs < 1 || Ws < 1) return CAVP_ERR_BAD_ARG;
  if (B > kAugMaxB || Hs > 16384 || Ws > 16384 || max_scale64 < 32 || max_scale64 > 256) return CAVP_ERR_UNSUPPORTED;
  const int mh = (int)(((long long)Hs * max_scale64) >> 6), mw = (int)(((long long)Ws * max_scale64) >> 6);
  const dim3 grid((mw + kAugTileW - 1) / kAugTileW, (mh + kAugTileH - 1) / kAugTileH, B);
  if (grid.y > 65535u) return CAVP_ERR_UNSUPPORTED;
  aug_resize_store_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(frames, sizes, Hs, Ws, mh, mw, jitter ? 1 : 0, params,
                                                                 (const unsigned long long*)lsum, scratch);
  CHECK_LAUNCH();
}

extern "C" int cavp_aug_resize_render(const void* src, int32_t src_is_frames, const uint8_t* masks, const int32_t* sizes, int32_t B,
                                      int32_t Hs, int32_t Ws, int32_t max_scale64, int32_t H, int32_t W, const float* mean3,
                                      const float* std3, const int32_t* params, const int32_t* near_tab, float* image, int64_t* label,
                                      void* stream) {
  if (!src || !masks || !sizes || !mean3 || !std3 || !params || !near_tab || !image || !label || !aug_shape_ok(B, Hs, Ws, H, W))
    return CAVP_ERR_BAD_ARG;
  if (!aug_resize_supported(B, Hs, Ws, H, W, src_is_frames ? 64 : max_scale64)) return CAVP_ERR_UNSUPPORTED;
  AugNorm nm;
  for (int c = 0; c < 3; ++c) {   // HOST arrays, passed by value as in cavp_aug_render; the variant has no pad, so no fill
    if (!(std3[c] > 0.0f)) return CAVP_ERR_BAD_ARG;
    nm.mean[c] = mean3[c];
    nm.std[c] = std3[c];
    nm.fill[c] = 0;
  }
  const dim3 grid((W + kAugTileW - 1) / kAugTileW, (H + kAugTileH - 1) / kAugTileH, B);
  if (grid.y > 65535u) return CAVP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (src_is_frames) {
    aug_resize_render_kernel<true><<<grid, 256, 0, s>>>((const unsigned char*)src, (long long)Hs * Ws * 3, Ws * 3, Hs, Ws, masks, sizes, Hs,
                                                        Ws, H, W, nm, params, near_tab, image, (long long*)label);
  } else {
    const int mh = (int)(((long long)Hs * max_scale64) >> 6), mw = (int)(((long long)Ws * max_scale64) >> 6);
    aug_resize_render_kernel<false><<<grid, 256, 0, s>>>((const unsigned char*)src, (long long)mh * mw * 4, mw * 4, mh, mw, masks, sizes,
                                                         Hs, Ws, H, W, nm, params, near_tab, image, (long long*)label);
  }
  CHECK_LAUNCH();
}
