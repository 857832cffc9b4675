// Deformable convolution, DCN v1 / v2: the bilinear gather that feeds the 1x1 conv GEMM, and the
// adjoints of the gather for the offsets, the mask and the input.
//
// Sampling is the project's own spec — the rule of mmdetection v1's modulated kernel — in strict IEEE fp32 in the
// spec's operation order: this file is compiled with -ffp-contract=off and every operation of the sample is __f*_rn.
// The CPU restatement is tests/deform_ref.py.
//
//   deform_sample_kernel       one thread per (output pixel, tap, 8 channels): four 16-byte corner loads from NHWC, one
//                              16-byte store into cols (N Ho Wo, 9 C), K index = tap * C + channel.
//   deform_coord_grad_kernel   per (pixel, deformable group, tap) the sums over the group's channels for d offset and
//                              d mask: L = 2^j lanes per item, each lane its channel groups in order, then a fixed
//                              xor tree over the L lanes.
//   deform_prep_kernel         input gradient 1/2: one 16-byte record per sample (top-left corner, fractions, mask value;
//                              -1 for an invalid sample) and the bounding box of every 256 records.
//   deform_input_grad_kernel   input gradient 2/2: one 256-thread workgroup per (image, 8x16-pixel tile, 64 channels).
//                              It walks the image's records in index order, 256 at a time (chunks whose box misses
//                              the tile are skipped), compacts those that reach the tile in order (wavefront ballot)
//                              and adds them into an fp32 LDS tile: a lane is a channel, wave w owns tile rows w and
//                              w + 4.  Every pixel is written once, zeros included.
// No float atomics and no inter-workgroup communication: each gradient element is one thread's sum in a fixed order (or
// a fixed tree over lanes), so the result is the same bits on every run, eager or replayed.
#include "common.h"
#include "conv_host.h"
#include <math.h>
#include <string.h>

#define DF_BLK 256
#define DF_TH 8         // tile rows: two per wavefront
#define DF_TW 16        // tile columns
#define DF_CS 64        // channels per workgroup: one per lane
#define DF_FAR (1 << 20)

struct DeformP {
  const bf16_t* x;
  const void* off;
  const void* msk;
  int64_t off_pitch, msk_pitch;
  int N, H, W, C, Ho, Wo, stride, pad, dg, Cg;
  int off_f32, msk_f32, logit;
};

// one sample, 16 bytes: (y0 + 1) | (x0 + 1) << 16, or -1; the bits of ly, lx and of the mask value (1 without a mask)
typedef __attribute__((ext_vector_type(4))) int DfRec;
struct DfBox {            // of the valid records of a chunk: rows [y_lo, y_hi], columns [x_lo, x_hi] of their (y0, x0)
  int y_lo, y_hi, x_lo, x_hi;
};

template <bool F16>
__device__ __forceinline__ float df_load(const void* p, int64_t i, int f32) {
  return f32 ? ((const float*)p)[i] : elem_to_f32<F16>(((const bf16_t*)p)[i]);
}
template <bool F16>
__device__ __forceinline__ void df_store(void* p, int64_t i, int f32, float v) {
  if (f32) ((float*)p)[i] = v;
  else ((bf16_t*)p)[i] = f32_to_elem<F16>(v);
}

// (the element goes through a scalar: a bit_cast applied directly to raw[c] reads element 0 for every c)
template <bool F16>
__device__ __forceinline__ void df_widen8(const s16x8_t raw, float* v) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const short e = raw[c];
    v[c] = elem_to_f32<F16>(__builtin_bit_cast(bf16_t, e));
  }
}

// ---- the spec, one function per step -------------------------------------------------------------------------
struct DfSamp {
  bool valid;
  int y0, x0;
  float ly, lx, hy, hx;
};
__device__ __forceinline__ DfSamp df_locate(const DeformP& P, int ho, int wo, int k, float dy, float dx) {
  const int i = k / 3, j = k - 3 * i;
  const float py = __fadd_rn((float)(ho * P.stride - P.pad + i * P.pad), dy);     // dilation == padding
  const float px = __fadd_rn((float)(wo * P.stride - P.pad + j * P.pad), dx);
  DfSamp s;
  s.valid = py > -1.f && py < (float)P.H && px > -1.f && px < (float)P.W;           // on the floats: NaN, inf -> false
  s.y0 = s.x0 = 0;
  s.ly = s.lx = s.hy = s.hx = 0.f;
  if (s.valid) {
    const float fy = floorf(py), fx = floorf(px);
    s.y0 = (int)fy;
    s.x0 = (int)fx;
    s.ly = __fsub_rn(py, fy);
    s.lx = __fsub_rn(px, fx);
    s.hy = __fsub_rn(1.f, s.ly);
    s.hx = __fsub_rn(1.f, s.lx);
  }
  return s;
}

template <bool F16>
__device__ __forceinline__ float df_mask(const DeformP& P, int64_t pix, int gk) {
  if (!P.msk) return 1.f;
  const float m = df_load<F16>(P.msk, pix * P.msk_pitch + gk, P.msk_f32);
  return P.logit ? __fdiv_rn(1.f, __fadd_rn(1.f, expf(-m))) : m;
}

// 8 channels of the corner (y, x) of one image; a corner outside the map is exactly 0
template <bool F16>
__device__ __forceinline__ void df_corner(const DeformP& P, const bf16_t* img, int y, int x, float* v) {
  if ((unsigned)y < (unsigned)P.H && (unsigned)x < (unsigned)P.W) {
    df_widen8<F16>(*(const s16x8_t*)(img + ((int64_t)y * P.W + x) * P.C), v);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = 0.f;
  }
}

__device__ __forceinline__ float df_bilinear(float w1, float w2, float w3, float w4, float v1, float v2, float v3,
                                             float v4) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, v1), __fmul_rn(w2, v2)), __fmul_rn(w3, v3)), __fmul_rn(w4, v4));
}

// ---- forward 1/2 ------------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(DF_BLK) void deform_sample_kernel(const DeformP P, bf16_t* __restrict__ cols) {
  const int CG = P.C / 8;
  const int64_t total = (int64_t)P.N * P.Ho * P.Wo * 9 * CG;
  for (int64_t q = blockIdx.x * (int64_t)DF_BLK + threadIdx.x; q < total; q += (int64_t)gridDim.x * DF_BLK) {
    const int cg = (int)(q % CG);
    int64_t t = q / CG;
    const int k = (int)(t % 9);
    const int64_t pix = t / 9;
    const int wo = (int)(pix % P.Wo);
    t = pix / P.Wo;
    const int ho = (int)(t % P.Ho);
    const int n = (int)(t / P.Ho);
    const int gk = (cg * 8 / P.Cg) * 9 + k;
    const int64_t ob = pix * P.off_pitch + 2 * gk;
    const DfSamp s = df_locate(P, ho, wo, k, df_load<F16>(P.off, ob, P.off_f32), df_load<F16>(P.off, ob + 1, P.off_f32));
    s16x8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s.valid) {
      const bf16_t* img = P.x + (int64_t)n * P.H * P.W * P.C + cg * 8;
      float v1[8], v2[8], v3[8], v4[8];
      df_corner<F16>(P, img, s.y0, s.x0, v1);
      df_corner<F16>(P, img, s.y0, s.x0 + 1, v2);
      df_corner<F16>(P, img, s.y0 + 1, s.x0, v3);
      df_corner<F16>(P, img, s.y0 + 1, s.x0 + 1, v4);
      const float w1 = __fmul_rn(s.hy, s.hx), w2 = __fmul_rn(s.hy, s.lx), w3 = __fmul_rn(s.ly, s.hx),
                  w4 = __fmul_rn(s.ly, s.lx);
      const float m = df_mask<F16>(P, pix, gk);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float val = df_bilinear(w1, w2, w3, w4, v1[c], v2[c], v3[c], v4[c]);
        if (P.msk) val = __fmul_rn(val, m);
        o[c] = __builtin_bit_cast(short, f32_to_elem<F16>(val));
      }
    }
    *(s16x8_t*)(cols + q * 8) = o;          // (pix, k, cg) row-major == (N Ho Wo, 9, C)
  }
}

// ---- weights: fp32 OIHW (any strides) -> w_fwd [O][k][c], w_dgrad [k][c][O] -------------------------------------------
template <bool F16>
__global__ void deform_pack_kernel(const float* __restrict__ w, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int O,
                                   int C, bf16_t* __restrict__ w_fwd, bf16_t* __restrict__ w_dgrad) {
  const int64_t total = (int64_t)O * 9 * C;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(q % C);
    const int k = (int)((q / C) % 9);
    const int o = (int)(q / ((int64_t)9 * C));
    const bf16_t v = f32_to_elem<F16>(w[o * s0 + c * s1 + (k / 3) * s2 + (k % 3) * s3]);
    w_fwd[q] = v;
    if (w_dgrad) w_dgrad[((int64_t)k * C + c) * O + o] = v;
  }
}

// ---- backward: offsets and mask -------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(DF_BLK) void deform_coord_grad_kernel(const DeformP P, const bf16_t* __restrict__ dcol,
                                                                    void* __restrict__ doff, void* __restrict__ dmsk,
                                                                    int lg) {
  const int L = 1 << lg;
  const int64_t items = (int64_t)P.N * P.Ho * P.Wo * P.dg * 9;
  const int64_t t = blockIdx.x * (int64_t)DF_BLK + threadIdx.x;
  const int64_t item = t >> lg;
  const int sub = (int)(t & (L - 1));
  const bool live = item < items;
  float sy = 0.f, sx = 0.f, sm = 0.f, m = 1.f;
  bool valid = false;
  int gk = 0;
  int64_t pix = 0;
  if (live) {
    const int k = (int)(item % 9);
    int64_t u = item / 9;
    const int g = (int)(u % P.dg);
    pix = u / P.dg;
    const int wo = (int)(pix % P.Wo);
    u = pix / P.Wo;
    const int ho = (int)(u % P.Ho);
    const int n = (int)(u / P.Ho);
    gk = g * 9 + k;
    const int64_t ob = pix * P.off_pitch + 2 * gk;
    const DfSamp s = df_locate(P, ho, wo, k, df_load<F16>(P.off, ob, P.off_f32), df_load<F16>(P.off, ob + 1, P.off_f32));
    valid = s.valid;
    if (valid) {
      m = df_mask<F16>(P, pix, gk);
      const float w1 = s.hy * s.hx, w2 = s.hy * s.lx, w3 = s.ly * s.hx, w4 = s.ly * s.lx;
      const bf16_t* img = P.x + (int64_t)n * P.H * P.W * P.C;
      const bf16_t* drow = dcol + (pix * 9 + k) * P.C;
      for (int j = sub; j < P.Cg / 8; j += L) {
        const int c = g * P.Cg + j * 8;
        float d[8], v1[8], v2[8], v3[8], v4[8];
        df_widen8<F16>(*(const s16x8_t*)(drow + c), d);
        df_corner<F16>(P, img + c, s.y0, s.x0, v1);
        df_corner<F16>(P, img + c, s.y0, s.x0 + 1, v2);
        df_corner<F16>(P, img + c, s.y0 + 1, s.x0, v3);
        df_corner<F16>(P, img + c, s.y0 + 1, s.x0 + 1, v4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          sy += d[e] * ((v3[e] - v1[e]) * s.hx + (v4[e] - v2[e]) * s.lx);
          sx += d[e] * ((v2[e] - v1[e]) * s.hy + (v4[e] - v3[e]) * s.ly);
          sm += d[e] * df_bilinear(w1, w2, w3, w4, v1[e], v2[e], v3[e], v4[e]);
        }
      }
    }
  }
  for (int o = L >> 1; o > 0; o >>= 1) {        // every lane of the wave takes part; partners hold the same sum after
    sy += __shfl_xor(sy, o);
    sx += __shfl_xor(sx, o);
    sm += __shfl_xor(sm, o);
  }
  if (live && sub == 0) {
    const int64_t ob = pix * P.off_pitch + 2 * gk;
    df_store<F16>(doff, ob, P.off_f32, valid ? m * sy : 0.f);
    df_store<F16>(doff, ob + 1, P.off_f32, valid ? m * sx : 0.f);
    if (dmsk) {
      if (P.logit) {        // s (1 - s) = t / (1 + t)^2, t = exp(-|logit|): no cancellation for a saturated sigmoid
        const float t = expf(-fabsf(df_load<F16>(P.msk, pix * P.msk_pitch + gk, P.msk_f32)));
        sm *= t / ((1.f + t) * (1.f + t));
      }
      df_store<F16>(dmsk, pix * P.msk_pitch + gk, P.msk_f32, valid ? sm : 0.f);
    }
  }
}

// ---- backward: input ------------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(DF_BLK) void deform_prep_kernel(const DeformP P, DfRec* __restrict__ rec,
                                                              DfBox* __restrict__ box, int chunks) {
  __shared__ int red[DF_BLK / 64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int64_t S = (int64_t)P.Ho * P.Wo * P.dg * 9;
  const int64_t s = (int64_t)ch * DF_BLK + tid;
  DfRec r = {-1, 0, 0, 0};
  int y_lo = DF_FAR, y_hi = -DF_FAR, x_lo = DF_FAR, x_hi = -DF_FAR;
  if (s < S) {
    const int k = (int)(s % 9);
    const int g = (int)((s / 9) % P.dg);
    const int p = (int)(s / (9 * P.dg));
    const int64_t pix = (int64_t)n * P.Ho * P.Wo + p;
    const int gk = g * 9 + k;
    const int64_t ob = pix * P.off_pitch + 2 * gk;
    const DfSamp q = df_locate(P, p / P.Wo, p % P.Wo, k, df_load<F16>(P.off, ob, P.off_f32),
                               df_load<F16>(P.off, ob + 1, P.off_f32));
    if (q.valid) {
      r[0] = (q.y0 + 1) | ((q.x0 + 1) << 16);
      r[1] = __float_as_int(q.ly);
      r[2] = __float_as_int(q.lx);
      r[3] = __float_as_int(df_mask<F16>(P, pix, gk));
      y_lo = y_hi = q.y0;
      x_lo = x_hi = q.x0;
    }
  }
  rec[(int64_t)blockIdx.x * DF_BLK + tid] = r;
  for (int o = 32; o > 0; o >>= 1) {
    y_lo = min(y_lo, __shfl_xor(y_lo, o));
    y_hi = max(y_hi, __shfl_xor(y_hi, o));
    x_lo = min(x_lo, __shfl_xor(x_lo, o));
    x_hi = max(x_hi, __shfl_xor(x_hi, o));
  }
  if (lane == 0) {
    red[wave][0] = y_lo;
    red[wave][1] = y_hi;
    red[wave][2] = x_lo;
    red[wave][3] = x_hi;
  }
  __syncthreads();
  if (tid == 0) {
    DfBox b = {red[0][0], red[0][1], red[0][2], red[0][3]};
    for (int w = 1; w < DF_BLK / 64; ++w) {
      b.y_lo = min(b.y_lo, red[w][0]);
      b.y_hi = max(b.y_hi, red[w][1]);
      b.x_lo = min(b.x_lo, red[w][2]);
      b.x_hi = max(b.x_hi, red[w][3]);
    }
    box[blockIdx.x] = b;
  }
}

template <bool F16>
__global__ __launch_bounds__(DF_BLK) void deform_input_grad_kernel(const DeformP P, const DfRec* __restrict__ rec,
                                                                    const DfBox* __restrict__ box,
                                                                    const bf16_t* __restrict__ dcol,
                                                                    bf16_t* __restrict__ dx, int chunks, int tiles_x,
                                                                    int tiles_y, int slices) {
  __shared__ float acc[DF_TH * DF_TW * DF_CS];
  __shared__ DfRec lrec[DF_BLK];
  __shared__ int lidx[DF_BLK];
  __shared__ unsigned long long cmask[DF_BLK / 64];
  __shared__ int wave_n[DF_BLK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int idx = (int)blockIdx.x;
  const int slice = idx % slices;
  idx /= slices;
  const int tx = idx % tiles_x;
  idx /= tiles_x;
  const int ty = idx % tiles_y;
  const int n = idx / tiles_y;
  const int ty0 = ty * DF_TH, tx0 = tx * DF_TW, c0 = slice * DF_CS;
  const int c = c0 + lane;
  const int gc = c / P.Cg, g_lo = c0 / P.Cg, g_hi = (c0 + DF_CS - 1) / P.Cg;
  const int H = P.H, W = P.W, dg = P.dg;
  for (int i = tid; i < DF_TH * DF_TW * DF_CS; i += DF_BLK) acc[i] = 0.f;
  const DfRec* irec = rec + (int64_t)n * chunks * DF_BLK;
  const DfBox* ibox = box + (int64_t)n * chunks;
  const bf16_t* dimg = dcol + (int64_t)n * P.Ho * P.Wo * 9 * P.C + c;

  for (int cb = 0; cb < chunks; cb += DF_BLK) {
    __syncthreads();                                       // acc is zero; cmask of the last round has been read
    bool near = false;
    if (cb + tid < chunks) {
      const DfBox b = ibox[cb + tid];
      near = b.y_hi + 1 >= ty0 && b.y_lo <= ty0 + DF_TH - 1 && b.x_hi + 1 >= tx0 && b.x_lo <= tx0 + DF_TW - 1;
    }
    const unsigned long long nm = __ballot(near);
    if (lane == 0) cmask[wave] = nm;
    __syncthreads();
    for (int cw = 0; cw < DF_BLK / 64; ++cw) {
      unsigned long long cm = cmask[cw];                   // the same in every thread
      while (cm) {
        const int chunk = cb + cw * 64 + (__ffsll((long long)cm) - 1);
        cm &= cm - 1;
        const int s0 = chunk * DF_BLK;
        const DfRec r = irec[(int64_t)s0 + tid];
        bool hit = false;
        if (r[0] >= 0) {
          const int y0 = (r[0] & 0xffff) - 1, x0 = (r[0] >> 16) - 1;
          const int g = ((s0 + tid) / 9) % dg;
          hit = y0 + 1 >= ty0 && y0 <= ty0 + DF_TH - 1 && x0 + 1 >= tx0 && x0 <= tx0 + DF_TW - 1 && g >= g_lo &&
                g <= g_hi;
        }
        const unsigned long long bm = __ballot(hit);
        if (lane == 0) wave_n[wave] = __popcll(bm);
        __syncthreads();
        int off = 0, cnt = 0;
#pragma unroll
        for (int w = 0; w < DF_BLK / 64; ++w) {
          off += w < wave ? wave_n[w] : 0;
          cnt += wave_n[w];
        }
        if (hit) {
          const int slot = off + __popcll(bm & ((1ull << lane) - 1ull));
          lrec[slot] = r;
          lidx[slot] = tid;
        }
        __syncthreads();
        for (int e = 0; e < cnt; ++e) {
          const DfRec q = lrec[e];
          const int y0 = (q[0] & 0xffff) - 1, x0 = (q[0] >> 16) - 1;
          const float ly = __int_as_float(q[1]), lx = __int_as_float(q[2]);
          const int r0 = y0 - ty0, r1 = r0 + 1;
          const bool own0 = (unsigned)r0 < (unsigned)DF_TH && (r0 & 3) == wave && y0 >= 0;
          const bool own1 = (unsigned)r1 < (unsigned)DF_TH && (r1 & 3) == wave && y0 + 1 < H;
          if (!own0 && !own1) continue;                    // wave-uniform
          const int s = s0 + lidx[e];
          const int k = s % 9, g = (s / 9) % dg, p = s / (9 * dg);
          if (g != gc) continue;                           // per lane only where a slice spans several groups
          const float gm = elem_to_f32<F16>(dimg[((int64_t)p * 9 + k) * P.C]) * __int_as_float(q[3]);
          const float hy = 1.f - ly, hx = 1.f - lx;
          const int q0 = x0 - tx0, q1 = q0 + 1;
          const bool in0 = (unsigned)q0 < (unsigned)DF_TW && x0 >= 0;
          const bool in1 = (unsigned)q1 < (unsigned)DF_TW && x0 + 1 < W;
          if (own0) {
            if (in0) acc[(r0 * DF_TW + q0) * DF_CS + lane] += gm * (hy * hx);
            if (in1) acc[(r0 * DF_TW + q1) * DF_CS + lane] += gm * (hy * lx);
          }
          if (own1) {
            if (in0) acc[(r1 * DF_TW + q0) * DF_CS + lane] += gm * (ly * hx);
            if (in1) acc[(r1 * DF_TW + q1) * DF_CS + lane] += gm * (ly * lx);
          }
        }
        __syncthreads();                                   // the list is rewritten by the next chunk
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < DF_TH * DF_TW * (DF_CS / 8); i += DF_BLK) {
    const int c8 = i % (DF_CS / 8), px = i / (DF_CS / 8);
    const int y = ty0 + px / DF_TW, x = tx0 + px % DF_TW;
    if (y < H && x < W) {
      s16x8_t v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = __builtin_bit_cast(short, f32_to_elem<F16>(acc[px * DF_CS + c8 * 8 + e]));
      *(s16x8_t*)(dx + (((int64_t)n * H + y) * W + x) * P.C + c0 + c8 * 8) = v;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------
static int deform_plan(const char* fn, const tdn_deform_desc* d, DeformP* P) {
  TDN_CHECK(d != nullptr, "%s: NULL descriptor", fn);
  TDN_CHECK(d->dtype == TDN_BF16 || d->dtype == TDN_F16, "%s: dtype %d is neither TDN_BF16 nor TDN_F16", fn, d->dtype);
  TDN_CHECK(d->offset_dtype == d->dtype || d->offset_dtype == TDN_F32, "%s: offsets must be float32 or the compute dtype",
            fn);
  TDN_CHECK(d->mask_dtype == d->dtype || d->mask_dtype == TDN_F32, "%s: the mask must be float32 or the compute dtype",
            fn);
  TDN_CHECK(d->stride == 1 || d->stride == 2, "%s: stride %d not supported (1 or 2)", fn, d->stride);
  TDN_CHECK(d->pad >= 1 && d->pad <= 32, "%s: pad %d not supported (3x3 with pad = dilation in 1..32)", fn, d->pad);
  TDN_CHECK(d->N >= 1 && d->H >= 1 && d->W >= 1 && d->H <= 32766 && d->W <= 32766, "%s: bad N x H x W %d x %d x %d", fn,
            d->N, d->H, d->W);
  const int dg = d->deformable_groups;
  TDN_CHECK(d->C >= 64 && d->C % 64 == 0, "%s: C = %d must be a positive multiple of 64", fn, d->C);
  TDN_CHECK(dg >= 1 && d->C % dg == 0 && (d->C / dg) % 8 == 0,
            "%s: %d deformable groups must divide C = %d into multiples of 8 channels", fn, dg, d->C);
  const int Ho = conv_out_sz(d->H, 3, d->stride, d->pad), Wo = conv_out_sz(d->W, 3, d->stride, d->pad);
  TDN_CHECK(Ho >= 1 && Wo >= 1, "%s: empty output", fn);
  TDN_CHECK((int64_t)d->N * Ho * Wo * 9 * dg < (1ll << 30) && (int64_t)d->N * d->H * d->W < (1ll << 30) &&
                (int64_t)d->N * Ho * Wo * 9 * (d->C / 8) < (1ll << 40),
            "%s: tensor too large", fn);
  TDN_CHECK(d->offset_pitch >= 18 * dg && (d->mask == nullptr || d->mask_pitch >= 9 * dg),
            "%s: offset / mask pitch below 18 / 9 channels per deformable group", fn);
  memset(P, 0, sizeof(*P));
  P->x = (const bf16_t*)d->x;
  P->off = d->offset;
  P->msk = d->mask;
  P->off_pitch = d->offset_pitch;
  P->msk_pitch = d->mask_pitch;
  P->N = d->N; P->H = d->H; P->W = d->W; P->C = d->C;
  P->Ho = Ho; P->Wo = Wo;
  P->stride = d->stride; P->pad = d->pad;
  P->dg = dg; P->Cg = d->C / dg;
  P->off_f32 = d->offset_dtype == TDN_F32;
  P->msk_f32 = d->mask_dtype == TDN_F32;
  P->logit = d->mask && d->mask_is_logit ? 1 : 0;
  return 0;
}

static int deform_ptrs(const char* fn, const tdn_deform_desc* d, bool need_x) {
  TDN_CHECK(d->offset != nullptr, "%s: NULL offsets", fn);
  TDN_CHECK(!need_x || (d->x && ((uintptr_t)d->x & 15) == 0), "%s: x must be non-NULL and 16-byte aligned", fn);
  return 0;
}

static int grid_of(int64_t n, int blk) { return tdn_grid_1d(n, blk, 65536); }

extern "C" int tdn_deform_sample(const tdn_deform_desc* d, void* cols, void* stream) {
  DeformP P;
  if (deform_plan("tdn_deform_sample", d, &P) != 0 || deform_ptrs("tdn_deform_sample", d, true) != 0) return -1;
  TDN_CHECK(cols && ((uintptr_t)cols & 15) == 0, "tdn_deform_sample: cols must be non-NULL and 16-byte aligned");
  const int64_t total = (int64_t)P.N * P.Ho * P.Wo * 9 * (P.C / 8);
  TDN_LAUNCH_T(deform_sample_kernel, d->dtype, dim3(grid_of(total, DF_BLK)), dim3(DF_BLK), stream, P, (bf16_t*)cols);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_pack_deform_weight(const float* w, int64_t s_o, int64_t s_i, int64_t s_h, int64_t s_w, int Cout,
                                      int C, void* w_fwd, void* w_dgrad, int dtype, void* stream) {
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(w && w_fwd, "tdn_pack_deform_weight: NULL pointer");
  TDN_CHECK(Cout >= 64 && Cout % 64 == 0 && C >= 64 && C % 64 == 0 && (int64_t)Cout * 9 * C < (1ll << 31),
            "tdn_pack_deform_weight: channels must be multiples of 64 (C=%d Cout=%d)", C, Cout);
  TDN_LAUNCH_T(deform_pack_kernel, dtype, dim3(grid_of((int64_t)Cout * 9 * C, 256)), dim3(256), stream, w, s_o, s_i,
               s_h, s_w, Cout, C, (bf16_t*)w_fwd, (bf16_t*)w_dgrad);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_deform_coord_grad(const tdn_deform_desc* d, const void* dcol, void* doffset, void* dmask,
                                     void* stream) {
  DeformP P;
  if (deform_plan("tdn_deform_coord_grad", d, &P) != 0 || deform_ptrs("tdn_deform_coord_grad", d, true) != 0) return -1;
  TDN_CHECK(dcol && ((uintptr_t)dcol & 15) == 0, "tdn_deform_coord_grad: dcol must be non-NULL and 16-byte aligned");
  TDN_CHECK(doffset && (dmask != nullptr) == (d->mask != nullptr),
            "tdn_deform_coord_grad: NULL doffset, or dmask given without a mask / missing with one");
  int lg = 0;
  while ((1 << lg) < P.Cg / 8 && lg < 6) ++lg;
  const int64_t blocks = (((int64_t)P.N * P.Ho * P.Wo * P.dg * 9) << lg) / DF_BLK + 1;
  TDN_CHECK(blocks < (1ll << 31), "tdn_deform_coord_grad: too many samples");
  TDN_LAUNCH_T(deform_coord_grad_kernel, d->dtype, dim3((unsigned)blocks), dim3(DF_BLK), stream, P,
               (const bf16_t*)dcol, doffset, dmask, lg);
  TDN_LAUNCH_CHECK();
  return 0;
}

struct DeformWs { DfRec* rec; DfBox* box; int64_t bytes; int chunks; };
static DeformWs deform_layout(int N, int Ho, int Wo, int dg, void* base) {   // a braced list is evaluated left to right
  const int64_t chunks = ((int64_t)Ho * Wo * dg * 9 + DF_BLK - 1) / DF_BLK;
  tdn_carver c{(char*)base, 0};
  return {c.take<DfRec>(N * chunks * DF_BLK), c.take<DfBox>(N * chunks), c.off, (int)chunks};
}
extern "C" int64_t tdn_deform_workspace_bytes(int N, int H, int W, int stride, int pad, int deformable_groups) {
  tdn_deform_desc d;
  memset(&d, 0, sizeof(d));
  d.N = N; d.H = H; d.W = W; d.C = 64 * (deformable_groups > 0 ? deformable_groups : 1);
  d.stride = stride; d.pad = pad; d.deformable_groups = deformable_groups;
  d.offset_pitch = 18ll * deformable_groups;
  DeformP P;
  if (deform_plan("tdn_deform_workspace_bytes", &d, &P) != 0) return -1;
  return deform_layout(N, P.Ho, P.Wo, P.dg, nullptr).bytes;
}

extern "C" int tdn_deform_input_grad(const tdn_deform_desc* d, const void* dcol, void* dx, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  DeformP P;
  if (deform_plan("tdn_deform_input_grad", d, &P) != 0 || deform_ptrs("tdn_deform_input_grad", d, false) != 0) return -1;
  TDN_CHECK(dcol && dx && ((uintptr_t)dx & 15) == 0, "tdn_deform_input_grad: dcol / dx must be non-NULL, dx 16-byte aligned");
  const DeformWs w = deform_layout(P.N, P.Ho, P.Wo, P.dg, workspace);
  if (tdn_check_ws("tdn_deform_input_grad", workspace, workspace_bytes, w.bytes) != 0) return -1;
  const int tiles_y = (P.H + DF_TH - 1) / DF_TH, tiles_x = (P.W + DF_TW - 1) / DF_TW, slices = P.C / DF_CS;
  const int64_t blocks = (int64_t)P.N * tiles_y * tiles_x * slices;
  TDN_CHECK(blocks < (1ll << 31) && (int64_t)P.N * w.chunks < (1ll << 31), "tdn_deform_input_grad: too many tiles");
  hipStream_t st = (hipStream_t)stream;
  TDN_LAUNCH_T(deform_prep_kernel, d->dtype, dim3(P.N * w.chunks), dim3(DF_BLK), st, P, w.rec, w.box, w.chunks);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH_T(deform_input_grad_kernel, d->dtype, dim3((unsigned)blocks), dim3(DF_BLK), st, P, (const DfRec*)w.rec,
               (const DfBox*)w.box, (const bf16_t*)dcol, (bf16_t*)dx, w.chunks, tiles_x, tiles_y, slices);
  TDN_LAUNCH_CHECK();
  return 0;
}
