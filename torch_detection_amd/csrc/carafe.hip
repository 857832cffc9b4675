// CARAFE content-aware upsampling (Wang et al., ICCV 2019): the reassembly gather, its feature gradient
// in gather form and its mask / logit gradient.  The CPU restatement is tests/carafe_ref.py.
//
//   out[n, c, ph, pw] = sum over taps t = i k + j, in that order, of  w[n, gi, t, ph, pw] * x[n, c, h - r + i, w - r + j]
//
// h = ph / s, w = pw / s, gi = c / (C / g), r = (k - 1) / 2; a tap outside the map is skipped.  The weights are either
// stored MASKS (N, sH, sW, >= g k^2; fp32 or 16-bit) or, template flag LOGITS, the softmax over the k^2 taps of the
// content encoder's output (N, H, W, >= g k^2 s^2), channel (gi k^2 + t) s^2 + dy s + dx — F.pixel_shuffle's rule — formed
// in the kernel:  p_t = exp(l_t - max) / sum_u exp(l_u - max), the sum in tap order.  Forward and backward evaluate that
// one expression, so they see the same weights bit for bit.
//
//   carafe_fwd_kernel   one workgroup per (image, TH x 8 tile of source pixels, group): the tile's weights once into LDS
//                       (softmax included), then per chunk of <= 64 channels the source patch plus halo into LDS and the
//                       taps from shifted 16-byte LDS reads; out = addend + sum in fp32, one rounding; only pixels inside
//                       the (Ho, Wo) crop are computed.
//   carafe_dx_kernel    one workgroup per (image, 8 x 8 tile of dx pixels, channel chunk): each dx element is ONE thread's
//                       sum over the (2r + 1)^2 source pixels that reach it, row-major, and their s^2 sub-pixels, row-major.
//                       LOGITS: (max, sum) of every (source pixel, sub-pixel) of tile + halo in LDS first.
//   carafe_dw_kernel    L = 2^j lanes per (image, source pixel, group): per tap the s^2 dot products over the group's
//                       channels (each lane its 8-channel vectors in order, then a fixed xor tree), kept in LDS; then the
//                       stores — LOGITS: p_t (dm_t - sum_u p_u dm_u) through the pixel-shuffle index.
// This file is compiled with -ffp-contract=off; the forward's operations are __f*_rn.  No atomics, no workspace, no host
// synchronisation: each output element is one thread's sum in a fixed order (or a fixed tree over lanes).
#include "common.h"
#include <math.h>
#include <string.h>

#define CF_BLK 256
#define CF_TW 8                      // tile columns (source pixels) of the forward; the dx tile is CF_TW x CF_TW
#define CF_WMAX 8192                 // fp32 weights of a forward tile: TH * 8 * s^2 * k^2 <= CF_WMAX
#define CF_PMAX (14 * 14 * 64)       // 16-bit elements of a patch: (8 + 6)^2 pixels of 64 channels
#define CF_SMAX (14 * 14 * 16 * 2)   // (max, sum) of tile + halo, s^2 <= 16
#define CF_DW_LDS 49152

struct CarafeP {
  const bf16_t* x;
  const void* wsrc;
  const bf16_t* addend;
  int64_t pitch;
  int N, C, H, W, k, r, s, g, Cg, k2, s2, sH, sW, Ho, Wo;
  int w_f32, cch, th;
};

template <bool F16>
__device__ __forceinline__ float cf_load(const void* p, int64_t i, int f32) {
  return f32 ? ((const float*)p)[i] : elem_to_f32<F16>(((const bf16_t*)p)[i]);
}
template <bool F16>
__device__ __forceinline__ void cf_store(void* p, int64_t i, int f32, float v) {
  if (f32) ((float*)p)[i] = v;
  else ((bf16_t*)p)[i] = f32_to_elem<F16>(v);
}
template <bool F16>
__device__ __forceinline__ void cf_widen8(const s16x8_t raw, float* v) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const short e = raw[c];
    v[c] = elem_to_f32<F16>(__builtin_bit_cast(bf16_t, e));
  }
}
template <bool F16>
__device__ __forceinline__ s16x8_t cf_narrow8(const float* v) {
  s16x8_t o;
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = __builtin_bit_cast(short, f32_to_elem<F16>(v[c]));
  return o;
}

// the softmax of one (source pixel, group, sub-pixel): `base` is the element index of tap 0, taps s2 elements apart
template <bool F16>
__device__ __forceinline__ void cf_stats(const CarafeP& P, int64_t base, float* mx, float* sum) {
  float m = cf_load<F16>(P.wsrc, base, P.w_f32);
  for (int t = 1; t < P.k2; ++t) m = fmaxf(m, cf_load<F16>(P.wsrc, base + (int64_t)t * P.s2, P.w_f32));
  float s = 0.f;
  for (int t = 0; t < P.k2; ++t)
    s = __fadd_rn(s, expf(__fsub_rn(cf_load<F16>(P.wsrc, base + (int64_t)t * P.s2, P.w_f32), m)));
  *mx = m;
  *sum = s;
}
__device__ __forceinline__ float cf_prob(float l, float mx, float sum) { return __fdiv_rn(expf(__fsub_rn(l, mx)), sum); }

__device__ __forceinline__ int64_t cf_logit_base(const CarafeP& P, int n, int h, int w, int gi, int q) {
  return (((int64_t)n * P.H + h) * P.W + w) * P.pitch + (int64_t)gi * P.k2 * P.s2 + q;
}
__device__ __forceinline__ int64_t cf_mask_base(const CarafeP& P, int n, int ph, int pw, int gi) {
  return (((int64_t)n * P.sH + ph) * P.sW + pw) * P.pitch + (int64_t)gi * P.k2;
}

// ---- forward -----------------------------------------------------------------------------------------------------
template <bool F16, bool LOGITS, int K>
__global__ __launch_bounds__(CF_BLK) void carafe_fwd_kernel(const CarafeP P, bf16_t* __restrict__ out, int tiles_x,
                                                             int tiles_y, int zs) {
  __shared__ float wl[CF_WMAX];                                      // [tile pixel][sub-pixel][tap]
  __shared__ __attribute__((aligned(16))) bf16_t patch[CF_PMAX];     // [patch pixel][8-channel vector][8]
  const int tid = threadIdx.x;
  int idx = (int)blockIdx.x;
  const int z = idx % zs;
  idx /= zs;
  const int gi = idx % P.g;
  idx /= P.g;
  const int tx = idx % tiles_x;
  idx /= tiles_x;
  const int ty = idx % tiles_y;
  const int n = idx / tiles_y;
  const int TH = P.th, TP = TH * CF_TW;
  const int h0 = ty * TH, w0 = tx * CF_TW;
  constexpr int k = K, r = (K - 1) / 2, k2 = K * K;
  const int s = P.s, s2 = P.s2;

  // a tap whose source pixel lies outside the map gets weight 0 here and meets a zero of the patch below: the sum is
  // the one that skips the tap (an accumulator that starts at +0 never becomes -0), whatever the stored weight holds
  if (LOGITS) {
    for (int e = tid; e < TP * s2; e += CF_BLK) {
      const int q = e % s2, p = e / s2;
      const int h = h0 + p / CF_TW, w = w0 + p % CF_TW;
      float* dst = wl + e * k2;
      if (h < P.H && w < P.W) {
        const int64_t base = cf_logit_base(P, n, h, w, gi, q);
        float mx, sum;
        cf_stats<F16>(P, base, &mx, &sum);
        for (int t = 0; t < k2; ++t) {
          const bool in = (unsigned)(h - r + t / k) < (unsigned)P.H && (unsigned)(w - r + t % k) < (unsigned)P.W;
          dst[t] = in ? cf_prob(cf_load<F16>(P.wsrc, base + (int64_t)t * s2, P.w_f32), mx, sum) : 0.f;
        }
      } else {
        for (int t = 0; t < k2; ++t) dst[t] = 0.f;
      }
    }
  } else {
    for (int e = tid; e < TP * s2 * k2; e += CF_BLK) {
      const int t = e % k2, pq = e / k2;
      const int q = pq % s2, p = pq / s2;
      const int h = h0 + p / CF_TW, w = w0 + p % CF_TW;
      const bool in = h < P.H && w < P.W && (unsigned)(h - r + t / k) < (unsigned)P.H &&
                      (unsigned)(w - r + t % k) < (unsigned)P.W;
      wl[e] = in ? cf_load<F16>(P.wsrc, cf_mask_base(P, n, h * s + q / s, w * s + q % s, gi) + t, P.w_f32) : 0.f;
    }
  }

  const int PW = CF_TW + 2 * r, PH = TH + 2 * r;
  const int nv = P.cch / 8, nchunks = P.Cg / P.cch;
  const bf16_t* img = P.x + (int64_t)n * P.H * P.W * P.C;
  for (int ch = z; ch < nchunks; ch += zs) {
    const int c0 = gi * P.Cg + ch * P.cch;
    __syncthreads();                                   // wl is complete; the last chunk's patch has been read
    for (int e = tid; e < PH * PW * nv; e += CF_BLK) {
      const int v = e % nv, pp = e / nv;
      const int y = h0 - r + pp / PW, x = w0 - r + pp % PW;
      s16x8_t val = {0, 0, 0, 0, 0, 0, 0, 0};
      if ((unsigned)y < (unsigned)P.H && (unsigned)x < (unsigned)P.W)
        val = *(const s16x8_t*)(img + ((int64_t)y * P.W + x) * P.C + c0 + v * 8);
      *(s16x8_t*)(patch + e * 8) = val;
    }
    __syncthreads();
    for (int it = tid; it < TP * s2 * nv; it += CF_BLK) {
      const int v = it % nv, pq = it / nv;
      const int q = pq % s2, p = pq / s2;
      const int py = p / CF_TW, px = p % CF_TW;
      const int h = h0 + py, w = w0 + px;
      const int ph = h * s + q / s, pw = w * s + q % s;
      if (h >= P.H || w >= P.W || ph >= P.Ho || pw >= P.Wo) continue;
      float acc[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] = 0.f;
      const float* wp = wl + pq * k2;
      const bf16_t* pb = patch + ((py * PW + px) * nv + v) * 8;
#pragma unroll
      for (int i = 0; i < k; ++i) {
#pragma unroll
        for (int j = 0; j < k; ++j) {
          const float m = wp[i * k + j];
          float xv[8];
          cf_widen8<F16>(*(const s16x8_t*)(pb + (i * PW + j) * nv * 8), xv);
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (LOGITS) acc[c] = __fmaf_rn(m, xv[c], acc[c]);      // held to the bound, not to bits: one rounding per tap
            else acc[c] = __fadd_rn(acc[c], __fmul_rn(m, xv[c]));
          }
        }
      }
      const int64_t o = (((int64_t)n * P.Ho + ph) * P.Wo + pw) * P.C + c0 + v * 8;
      if (P.addend) {
        float a[8];
        cf_widen8<F16>(*(const s16x8_t*)(P.addend + o), a);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __fadd_rn(a[c], acc[c]);
      }
      *(s16x8_t*)(out + o) = cf_narrow8<F16>(acc);
    }
  }
}

// ---- feature gradient ----------------------------------------------------------------------------------------------
template <bool F16, bool LOGITS>
__global__ __launch_bounds__(CF_BLK) void carafe_dx_kernel(const CarafeP P, const bf16_t* __restrict__ gout,
                                                            bf16_t* __restrict__ dx, int tiles_x, int tiles_y) {
  extern __shared__ float cf_dx_dyn[];                 // LOGITS: [halo pixel][sub-pixel](max, sum)
  float* st = cf_dx_dyn;
  const int tid = threadIdx.x;
  const int chunks = P.C / P.cch;
  int idx = (int)blockIdx.x;
  const int ch = idx % chunks;
  idx /= chunks;
  const int tx = idx % tiles_x;
  idx /= tiles_x;
  const int ty = idx % tiles_y;
  const int n = idx / tiles_y;
  const int c0 = ch * P.cch, gi = c0 / P.Cg;
  const int h0 = ty * CF_TW, w0 = tx * CF_TW;
  const int k = P.k, r = P.r, s = P.s, s2 = P.s2;
  const int PW = CF_TW + 2 * r;
  if (LOGITS) {
    for (int e = tid; e < PW * PW * s2; e += CF_BLK) {
      const int q = e % s2, pp = e / s2;
      const int y = h0 - r + pp / PW, x = w0 - r + pp % PW;
      float mx = 0.f, sum = 1.f;
      if ((unsigned)y < (unsigned)P.H && (unsigned)x < (unsigned)P.W) cf_stats<F16>(P, cf_logit_base(P, n, y, x, gi, q), &mx, &sum);
      st[2 * e] = mx;
      st[2 * e + 1] = sum;
    }
    __syncthreads();
  }
  const int nv = P.cch / 8;
  for (int it = tid; it < CF_TW * CF_TW * nv; it += CF_BLK) {
    const int v = it % nv, p = it / nv;
    const int h = h0 + p / CF_TW, w = w0 + p % CF_TW;
    if (h >= P.H || w >= P.W) continue;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    const int h_lo = max(h - r, 0), h_hi = min(h + r, P.H - 1), w_lo = max(w - r, 0), w_hi = min(w + r, P.W - 1);
    for (int h2 = h_lo; h2 <= h_hi; ++h2) {
      for (int w2 = w_lo; w2 <= w_hi; ++w2) {
        const int t = (h - h2 + r) * k + (w - w2 + r);
        const int pp = (h2 - h0 + r) * PW + (w2 - w0 + r);
        for (int q = 0; q < s2; ++q) {
          const int ph = s * h2 + q / s, pw = s * w2 + q % s;
          if (ph >= P.Ho || pw >= P.Wo) continue;
          float m;
          if (LOGITS) {
            const float l = cf_load<F16>(P.wsrc, cf_logit_base(P, n, h2, w2, gi, q) + (int64_t)t * s2, P.w_f32);
            m = cf_prob(l, st[2 * (pp * s2 + q)], st[2 * (pp * s2 + q) + 1]);
          } else {
            m = cf_load<F16>(P.wsrc, cf_mask_base(P, n, ph, pw, gi) + t, P.w_f32);
          }
          float gv[8];
          cf_widen8<F16>(*(const s16x8_t*)(gout + (((int64_t)n * P.Ho + ph) * P.Wo + pw) * P.C + c0 + v * 8), gv);
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(gv[c], m));
        }
      }
    }
    *(s16x8_t*)(dx + (((int64_t)n * P.H + h) * P.W + w) * P.C + c0 + v * 8) = cf_narrow8<F16>(acc);
  }
}

// ---- mask / logit gradient -----------------------------------------------------------------------------------------
template <bool F16, bool LOGITS>
__global__ __launch_bounds__(CF_BLK) void carafe_dw_kernel(const CarafeP P, const bf16_t* __restrict__ gout,
                                                            void* __restrict__ dwt, int lg, int64_t items) {
  extern __shared__ float cf_dyn[];                    // dm [item][sub-pixel][tap] | (max, sum, dot) [item][sub-pixel]
  const int L = 1 << lg, ipb = CF_BLK >> lg;
  const int k = P.k, r = P.r, s = P.s, k2 = P.k2, s2 = P.s2;
  const int tid = threadIdx.x, sub = tid & (L - 1), il = tid >> lg;
  const int64_t item = blockIdx.x * (int64_t)ipb + il;
  const bool live = item < items;
  int gi = 0, n = 0, h = 0, w = 0;
  if (live) {
    gi = (int)(item % P.g);
    int64_t u = item / P.g;
    w = (int)(u % P.W);
    u /= P.W;
    h = (int)(u % P.H);
    n = (int)(u / P.H);
  }
  float* dm = cf_dyn + il * s2 * k2;
  float* stt = cf_dyn + ipb * s2 * k2 + il * s2 * 3;
  const int nvec = P.Cg / 8;
  const bf16_t* img = P.x + (int64_t)n * P.H * P.W * P.C + gi * P.Cg;
  const bf16_t* gimg = gout + (int64_t)n * P.Ho * P.Wo * P.C + gi * P.Cg;
  for (int t = 0; t < k2; ++t) {
    float acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const int yy = h - r + t / k, xx = w - r + t % k;
    if (live && (unsigned)yy < (unsigned)P.H && (unsigned)xx < (unsigned)P.W) {
      for (int j = sub; j < nvec; j += L) {
        float xv[8];
        cf_widen8<F16>(*(const s16x8_t*)(img + ((int64_t)yy * P.W + xx) * P.C + j * 8), xv);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          if (q < s2) {
            const int ph = h * s + q / s, pw = w * s + q % s;
            if (ph < P.Ho && pw < P.Wo) {
              float gv[8];
              cf_widen8<F16>(*(const s16x8_t*)(gimg + ((int64_t)ph * P.Wo + pw) * P.C + j * 8), gv);
#pragma unroll
              for (int c = 0; c < 8; ++c) acc[q] += gv[c] * xv[c];
            }
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (q < s2) {                                    // s2 is uniform: every lane of the wave takes part
        for (int o = L >> 1; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o);
        if (live && sub == 0) dm[q * k2 + t] = acc[q];
      }
    }
  }
  __syncthreads();
  if (LOGITS) {
    if (live) {
      for (int q = sub; q < s2; q += L) {
        const int64_t base = cf_logit_base(P, n, h, w, gi, q);
        float mx, sum, dot = 0.f;
        cf_stats<F16>(P, base, &mx, &sum);
        for (int t = 0; t < k2; ++t)
          dot += cf_prob(cf_load<F16>(P.wsrc, base + (int64_t)t * s2, P.w_f32), mx, sum) * dm[q * k2 + t];
        stt[q * 3] = mx;
        stt[q * 3 + 1] = sum;
        stt[q * 3 + 2] = dot;
      }
    }
    __syncthreads();
    if (live) {
      const int64_t base = cf_logit_base(P, n, h, w, gi, 0);
      for (int e = sub; e < s2 * k2; e += L) {         // e = t s2 + q: the logits' own channel order
        const int q = e % s2, t = e / s2;
        const float p = cf_prob(cf_load<F16>(P.wsrc, base + e, P.w_f32), stt[q * 3], stt[q * 3 + 1]);
        cf_store<F16>(dwt, base + e, P.w_f32, p * (dm[q * k2 + t] - stt[q * 3 + 2]));
      }
    }
  } else {
    if (live) {
      for (int e = sub; e < s2 * k2; e += L) {
        const int t = e % k2, q = e / k2;
        cf_store<F16>(dwt, cf_mask_base(P, n, h * s + q / s, w * s + q % s, gi) + t, P.w_f32, dm[q * k2 + t]);
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------
static int carafe_plan(const char* fn, const tdn_carafe_desc* d, CarafeP* P) {
  TDN_CHECK(d != nullptr, "%s: NULL descriptor", fn);
  TDN_CHECK(d->dtype == TDN_BF16 || d->dtype == TDN_F16, "%s: dtype %d is neither TDN_BF16 nor TDN_F16", fn, d->dtype);
  TDN_CHECK(d->weight_dtype == d->dtype || d->weight_dtype == TDN_F32,
            "%s: masks / logits must be float32 or the compute dtype", fn);
  const int k = d->kernel_size, s = d->scale_factor, g = d->group_size;
  TDN_CHECK(k >= 1 && k <= 7 && (k & 1), "%s: kernel_size %d not supported (odd, 1..7)", fn, k);
  TDN_CHECK(s >= 1 && s <= 4, "%s: scale_factor %d not supported (1..4)", fn, s);
  TDN_CHECK(g >= 1 && (int64_t)g * k * k * s * s <= 1024, "%s: group_size * kernel_size^2 * scale_factor^2 must be in 1..1024", fn);
  TDN_CHECK(d->N >= 1 && d->H >= 1 && d->W >= 1 && d->H <= 32766 && d->W <= 32766, "%s: bad N x H x W %d x %d x %d", fn,
            d->N, d->H, d->W);
  TDN_CHECK((int64_t)d->N * d->H * s * d->W * s < (1ll << 30), "%s: tensor too large (N sH sW must be below 2^30)", fn);
  TDN_CHECK(d->C >= 64 && d->C % 64 == 0, "%s: C = %d must be a positive multiple of 64", fn, d->C);
  TDN_CHECK(d->C % g == 0 && (d->C / g) % 8 == 0, "%s: group_size %d must divide C = %d into multiples of 8 channels", fn,
            g, d->C);
  const int sH = d->H * s, sW = d->W * s;
  TDN_CHECK(d->out_h > sH - s && d->out_h <= sH && d->out_w > sW - s && d->out_w <= sW,
            "%s: out_size %d x %d outside (%d..%d) x (%d..%d)", fn, d->out_h, d->out_w, sH - s + 1, sH, sW - s + 1, sW);
  const int ch = g * k * k * (d->weights_are_logits ? s * s : 1);
  TDN_CHECK(d->weights != nullptr && d->weight_pitch >= ch, "%s: NULL masks / logits, or pitch below %d channels", fn, ch);
  memset(P, 0, sizeof(*P));
  P->x = (const bf16_t*)d->x;
  P->wsrc = d->weights;
  P->addend = (const bf16_t*)d->addend;
  P->pitch = d->weight_pitch;
  P->N = d->N; P->C = d->C; P->H = d->H; P->W = d->W;
  P->k = k; P->r = (k - 1) / 2; P->s = s; P->g = g; P->Cg = d->C / g; P->k2 = k * k; P->s2 = s * s;
  P->sH = sH; P->sW = sW; P->Ho = d->out_h; P->Wo = d->out_w;
  P->w_f32 = d->weight_dtype == TDN_F32;
  P->cch = 64;
  while (P->Cg % P->cch) P->cch >>= 1;               // 64, 32, 16 or 8: Cg is a multiple of 8
  P->th = 8;
  while (P->th > 1 && P->th * CF_TW * P->s2 * P->k2 > CF_WMAX) P->th >>= 1;
  TDN_CHECK(P->th * CF_TW * P->s2 * P->k2 <= CF_WMAX && (P->th + 2 * P->r) * (CF_TW + 2 * P->r) * P->cch <= CF_PMAX &&
                (CF_TW + 2 * P->r) * (CF_TW + 2 * P->r) * P->s2 * 2 <= CF_SMAX,
            "%s: internal: tile does not fit", fn);
  return 0;
}

static bool cf_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

#define CF_LAUNCH(kernel, d, grid, lds, stream, ...)                                                          \
  do {                                                                                                        \
    const bool f16_ = (d)->dtype == TDN_F16, lg_ = (d)->weights_are_logits != 0;                              \
    if (f16_ && lg_) TDN_LAUNCH((kernel<true, true>), grid, dim3(CF_BLK), lds, stream, __VA_ARGS__);          \
    else if (f16_) TDN_LAUNCH((kernel<true, false>), grid, dim3(CF_BLK), lds, stream, __VA_ARGS__);           \
    else if (lg_) TDN_LAUNCH((kernel<false, true>), grid, dim3(CF_BLK), lds, stream, __VA_ARGS__);            \
    else TDN_LAUNCH((kernel<false, false>), grid, dim3(CF_BLK), lds, stream, __VA_ARGS__);                    \
  } while (0)

#define CF_LAUNCH_K(kernel, K, d, grid, stream, ...)                                                          \
  do {                                                                                                        \
    const bool f16_ = (d)->dtype == TDN_F16, lg_ = (d)->weights_are_logits != 0;                              \
    if (f16_ && lg_) TDN_LAUNCH((kernel<true, true, K>), grid, dim3(CF_BLK), 0, stream, __VA_ARGS__);         \
    else if (f16_) TDN_LAUNCH((kernel<true, false, K>), grid, dim3(CF_BLK), 0, stream, __VA_ARGS__);          \
    else if (lg_) TDN_LAUNCH((kernel<false, true, K>), grid, dim3(CF_BLK), 0, stream, __VA_ARGS__);           \
    else TDN_LAUNCH((kernel<false, false, K>), grid, dim3(CF_BLK), 0, stream, __VA_ARGS__);                   \
  } while (0)

extern "C" int tdn_carafe_forward(const tdn_carafe_desc* d, void* out, void* stream) {
  CarafeP P;
  if (carafe_plan("tdn_carafe_forward", d, &P) != 0) return -1;
  TDN_CHECK(cf_aligned(d->x) && cf_aligned(out) && (d->addend == nullptr || cf_aligned(d->addend)),
            "tdn_carafe_forward: x, out (and addend) must be non-NULL and 16-byte aligned");
  const int tiles_y = ceil_div(P.H, P.th), tiles_x = ceil_div(P.W, CF_TW);
  const int64_t base = (int64_t)P.N * tiles_y * tiles_x * P.g;
  const int zs = base < 1024 ? P.Cg / P.cch : 1;      // few tiles: the channel chunks of a group go to workgroups of their own
  TDN_CHECK(base * zs < (1ll << 31), "tdn_carafe_forward: too many tiles");
  const dim3 grid((unsigned)(base * zs));
  bf16_t* o = (bf16_t*)out;
  switch (P.k) {                                      // the tap loops are unrolled: one instantiation per kernel size
    case 1: CF_LAUNCH_K(carafe_fwd_kernel, 1, d, grid, stream, P, o, tiles_x, tiles_y, zs); break;
    case 3: CF_LAUNCH_K(carafe_fwd_kernel, 3, d, grid, stream, P, o, tiles_x, tiles_y, zs); break;
    case 5: CF_LAUNCH_K(carafe_fwd_kernel, 5, d, grid, stream, P, o, tiles_x, tiles_y, zs); break;
    default: CF_LAUNCH_K(carafe_fwd_kernel, 7, d, grid, stream, P, o, tiles_x, tiles_y, zs); break;
  }
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_carafe_feature_grad(const tdn_carafe_desc* d, const void* gout, void* dx, void* stream) {
  CarafeP P;
  if (carafe_plan("tdn_carafe_feature_grad", d, &P) != 0) return -1;
  TDN_CHECK(cf_aligned(gout) && cf_aligned(dx), "tdn_carafe_feature_grad: gout and dx must be non-NULL and 16-byte aligned");
  const int tiles_y = ceil_div(P.H, CF_TW), tiles_x = ceil_div(P.W, CF_TW);
  const int lds = d->weights_are_logits ? (CF_TW + 2 * P.r) * (CF_TW + 2 * P.r) * P.s2 * 2 * (int)sizeof(float) : 0;
  const int64_t blocks = (int64_t)P.N * tiles_y * tiles_x * (P.C / P.cch);
  TDN_CHECK(blocks < (1ll << 31), "tdn_carafe_feature_grad: too many tiles");
  CF_LAUNCH(carafe_dx_kernel, d, dim3((unsigned)blocks), lds, stream, P, (const bf16_t*)gout, (bf16_t*)dx, tiles_x, tiles_y);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_carafe_mask_grad(const tdn_carafe_desc* d, const void* gout, void* dweights, void* stream) {
  CarafeP P;
  if (carafe_plan("tdn_carafe_mask_grad", d, &P) != 0) return -1;
  TDN_CHECK(cf_aligned(d->x) && cf_aligned(gout) && dweights,
            "tdn_carafe_mask_grad: x and gout must be non-NULL and 16-byte aligned, dweights non-NULL");
  int lg = 2;
  while ((1 << lg) < P.Cg / 8 && lg < 6) ++lg;
  const int per_item = P.s2 * (P.k2 + 3) * (int)sizeof(float);
  while ((CF_BLK >> lg) * per_item > CF_DW_LDS && lg < 6) ++lg;
  const int lds = (CF_BLK >> lg) * per_item;
  TDN_CHECK(lds <= CF_DW_LDS, "tdn_carafe_mask_grad: internal: LDS");
  const int64_t items = (int64_t)P.N * P.H * P.W * P.g;
  const int ipb = CF_BLK >> lg;
  const int64_t blocks = (items + ipb - 1) / ipb;
  TDN_CHECK(blocks < (1ll << 31), "tdn_carafe_mask_grad: too many pixels");
  CF_LAUNCH(carafe_dw_kernel, d, dim3((unsigned)blocks), lds, stream, P, (const bf16_t*)gout, dweights, lg, items);
  TDN_LAUNCH_CHECK();
  return 0;
}
