// Multi-level RoIAlign — the FPN RoI extractor — forward and backward.
//
// Semantics are the project's own spec in the mmdetection-v1 lineage (SingleRoIExtractor + RoIAlign, aligned=False,
// '+1' ends), strict IEEE fp32 in the spec's operation order: this file is compiled with -ffp-contract=off and every
// product, quotient and sum is __f*_rn.  The CPU restatement is tests/roi_ref.py.
//
//   roi_align_fwd_kernel   one thread per (row, bin, 8 channels): level mapping, geometry, the bin's samples
//                          (4 corner loads of 16 bytes each from NHWC), one rounding to the 16-bit type.  One launch
//                          for every level and image; invalid rows write zeros.
//   roi_prep_kernel        backward 1/2: per row its (level, image) key, the feature rows / columns its corners can
//                          touch and its geometry, into the workspace.
//   roi_align_bwd_kernel   backward 2/2: one 256-thread workgroup per (level, image, 4x16-pixel tile, 256 channels).
//                          It walks the rows in index order, keeps those whose key matches and whose reach overlaps
//                          the tile (ordered compaction through a wavefront ballot) and adds their terms into
//                          registers: wave w owns tile row w, a lane owns 8 pixels x 8 channels.  Every pixel of
//                          every level is written once, zeros included.
// No float atomics and no inter-workgroup communication: each gradient element is one thread's sum in a fixed order,
// so the result is the same bits on every run, eager or replayed.
#include "common.h"
#include <math.h>
#include <string.h>

#define ROI_BLK 256
#define BWD_TH 4        // tile rows: one per wavefront
#define BWD_TW 16       // tile columns: two lanes' 8 each
#define BWD_CG 32       // 8-channel groups per workgroup (256 channels)

struct RoiLevels {
  bf16_t* ptr[TDN_ROI_MAX_LEVELS];
  int64_t sn[TDN_ROI_MAX_LEVELS], sh[TDN_ROI_MAX_LEVELS], sw[TDN_ROI_MAX_LEVELS];
  int H[TDN_ROI_MAX_LEVELS], W[TDN_ROI_MAX_LEVELS];
  float scale[TDN_ROI_MAX_LEVELS];
  int blk_off[TDN_ROI_MAX_LEVELS + 1];   // backward: first workgroup of each level
  int tiles_x[TDN_ROI_MAX_LEVELS], tiles_y[TDN_ROI_MAX_LEVELS];
  int L, B, C, CG, S, sr, nchunk;
  float finest;
};

// ---- the spec, one function per step -------------------------------------------------------------------------
__device__ __forceinline__ bool roi_batch(float bf, int B, int* b) {
  if (!(bf > -1.f && bf < (float)B)) return false;     // truncation lands outside [0, B) (NaN too)
  *b = (int)bf;
  return true;
}

// floor(log2(s)) from the exponent of s; non-positive or non-normal s -> 0; clamped to [0, L-1]
__device__ __forceinline__ int roi_level(float x1, float y1, float x2, float y2, float finest, int L) {
  const float w = __fadd_rn(__fsub_rn(x2, x1), 1.f), h = __fadd_rn(__fsub_rn(y2, y1), 1.f);
  const float scale = __fsqrt_rn(__fmul_rn(w, h));
  const float s = __fadd_rn(__fdiv_rn(scale, finest), 1e-6f);
  const uint32_t u = __float_as_uint(s);
  const int e = (int)((u >> 23) & 0xffu);
  if ((u >> 31) || e == 0 || e == 255) return 0;
  const int lvl = e - 127;
  return lvl < 0 ? 0 : (lvl > L - 1 ? L - 1 : lvl);
}

__device__ __forceinline__ int roi_samples(float bin) {
  const float c = ceilf(bin);
  return c < (float)TDN_ROI_MAX_SAMPLES ? (int)c : TDN_ROI_MAX_SAMPLES;
}

struct RoiGeom {
  float sw, sh, bw, bh;
  int gw, gh;
};
__device__ __forceinline__ RoiGeom roi_geom(float x1, float y1, float x2, float y2, float sc, int S, int sr) {
  RoiGeom g;
  g.sw = __fmul_rn(x1, sc);
  g.sh = __fmul_rn(y1, sc);
  const float ew = __fmul_rn(__fadd_rn(x2, 1.f), sc), eh = __fmul_rn(__fadd_rn(y2, 1.f), sc);
  float rw = __fsub_rn(ew, g.sw), rh = __fsub_rn(eh, g.sh);
  rw = rw > 0.f ? rw : 0.f;
  rh = rh > 0.f ? rh : 0.f;
  g.bw = __fdiv_rn(rw, (float)S);
  g.bh = __fdiv_rn(rh, (float)S);
  g.gw = sr > 0 ? sr : roi_samples(g.bw);
  g.gh = sr > 0 ? sr : roi_samples(g.bh);
  return g;
}

// (s0 + p*bin) + ((i + 0.5) * bin) / g
__device__ __forceinline__ float roi_sample(float s0, int p, float bin, int i, int g) {
  return __fadd_rn(__fadd_rn(s0, __fmul_rn((float)p, bin)), __fdiv_rn(__fmul_rn(__fadd_rn((float)i, 0.5f), bin),
                                                                      (float)g));
}

// one axis of bilinear_interpolate, after the caller's range check (v in [-1, n])
struct Axis {
  int lo, hi;
  float l, h;
};
__device__ __forceinline__ Axis roi_axis(float v, int n) {
  Axis a;
  v = v > 0.f ? v : 0.f;
  a.lo = (int)v;
  if (a.lo >= n - 1) {
    a.lo = a.hi = n - 1;
    v = (float)a.lo;
  } else {
    a.hi = a.lo + 1;
  }
  a.l = __fsub_rn(v, (float)a.lo);
  a.h = __fsub_rn(1.f, a.l);
  return a;
}

// (the element goes through a scalar: a bit_cast applied directly to raw[c] reads element 0 for every c)
template <bool F16>
__device__ __forceinline__ void widen8(const s16x8_t raw, float* v) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const short e = raw[c];
    v[c] = elem_to_f32<F16>(__builtin_bit_cast(bf16_t, e));
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(ROI_BLK) void roi_align_fwd_kernel(const RoiLevels P, const float* __restrict__ rois,
                                                                 int64_t R, bf16_t* __restrict__ out) {
  const int S = P.S, CG = P.CG;
  const int64_t total = R * S * S * CG;
  for (int64_t q = blockIdx.x * (int64_t)ROI_BLK + threadIdx.x; q < total; q += (int64_t)gridDim.x * ROI_BLK) {
    const int cg = (int)(q % CG);
    int64_t t = q / CG;
    const int pw = (int)(t % S);
    t /= S;
    const int ph = (int)(t % S);
    const int64_t r = t / S;
    const float* rr = rois + r * 5;
    s16x8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
    int b;
    if (roi_batch(rr[0], P.B, &b)) {
      const float x1 = rr[1], y1 = rr[2], x2 = rr[3], y2 = rr[4];
      const int l = roi_level(x1, y1, x2, y2, P.finest, P.L);
      const RoiGeom g = roi_geom(x1, y1, x2, y2, P.scale[l], S, P.sr);
      const int H = P.H[l], W = P.W[l];
      const float Hf = (float)H, Wf = (float)W;
      const bf16_t* base = P.ptr[l] + b * P.sn[l] + cg * 8;
      const int64_t sh = P.sh[l], sw = P.sw[l];
      float acc[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] = 0.f;
      for (int iy = 0; iy < g.gh; ++iy) {
        const float y = roi_sample(g.sh, ph, g.bh, iy, g.gh);
        const bool yok = !(y < -1.f || y > Hf);
        const Axis ay = roi_axis(yok ? y : 0.f, H);
        for (int ix = 0; ix < g.gw; ++ix) {
          const float x = roi_sample(g.sw, pw, g.bw, ix, g.gw);
          if (!yok || x < -1.f || x > Wf) continue;          // value 0: acc + 0 == acc (acc is never -0)
          const Axis ax = roi_axis(x, W);
          const float w1 = __fmul_rn(ay.h, ax.h), w2 = __fmul_rn(ay.h, ax.l), w3 = __fmul_rn(ay.l, ax.h),
                      w4 = __fmul_rn(ay.l, ax.l);
          float v1[8], v2[8], v3[8], v4[8];
          widen8<F16>(*(const s16x8_t*)(base + ay.lo * sh + ax.lo * sw), v1);
          widen8<F16>(*(const s16x8_t*)(base + ay.lo * sh + ax.hi * sw), v2);
          widen8<F16>(*(const s16x8_t*)(base + ay.hi * sh + ax.lo * sw), v3);
          widen8<F16>(*(const s16x8_t*)(base + ay.hi * sh + ax.hi * sw), v4);
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const float val = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, v1[c]), __fmul_rn(w2, v2[c])),
                                                  __fmul_rn(w3, v3[c])), __fmul_rn(w4, v4[c]));
            acc[c] = __fadd_rn(acc[c], val);
          }
        }
      }
      const int n = g.gh * g.gw;
      const float cnt = (float)(n > 1 ? n : 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) o[c] = __builtin_bit_cast(short, f32_to_elem<F16>(__fdiv_rn(acc[c], cnt)));
    }
    *(s16x8_t*)(out + q * 8) = o;     // (r, ph, pw, cg) row-major == (R, S, S, C)
  }
}

__global__ void roi_map_levels_kernel(const float* __restrict__ rois, int64_t R, int L, float finest,
                                      int64_t* __restrict__ levels) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
    const float* rr = rois + r * 5;
    levels[r] = roi_level(rr[1], rr[2], rr[3], rr[4], finest, L);
  }
}

__global__ void rois_from_proposals_kernel(const float* __restrict__ prop, const int32_t* __restrict__ counts,
                                           int B, int M, float* __restrict__ rois) {
  const int64_t total = (int64_t)B * M;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / M), m = (int)(i % M);
    const float* p = prop + i * 5;
    float* o = rois + i * 5;
    o[0] = m < counts[b] ? (float)b : -1.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e + 1] = p[e];
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
// workspace records of a row: key (level << 16 | image, or -1), reach rows [lo, hi] / cols [lo, hi] (every corner
// any of its samples can touch lies inside), samples per side, geometry
struct RoiRec {
  int key, r0, r1, c0, c1, gh, gw, pad;
};

__device__ __forceinline__ int reach_lo(float s) {     // corners of samples >= s are >= floor(s) - 1 (margin 4)
  float f = floorf(s) - 4.f;
  if (!(f >= -8.f)) f = -8.f;                           // also NaN: a NaN sample clamps to 0
  return f < 1e6f ? (int)f : 1000000;
}
__device__ __forceinline__ int reach_hi(float e) {     // corners of samples <= e are <= floor(e) + 2 (margin 5)
  float f = ceilf(e) + 5.f;
  if (!(f <= 1e6f)) f = 1e6f;
  return f > -8.f ? (int)f : -8;
}

__global__ void roi_prep_kernel(const RoiLevels P, const float* __restrict__ rois, int64_t R, RoiRec* __restrict__ rec,
                                f32x4_t* __restrict__ geo) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
    const float* rr = rois + r * 5;
    RoiRec o = {-1, 0, -1, 0, -1, 0, 0, 0};
    f32x4_t gv = {0.f, 0.f, 0.f, 0.f};
    int b;
    if (roi_batch(rr[0], P.B, &b)) {
      const float x1 = rr[1], y1 = rr[2], x2 = rr[3], y2 = rr[4];
      const int l = roi_level(x1, y1, x2, y2, P.finest, P.L);
      const RoiGeom g = roi_geom(x1, y1, x2, y2, P.scale[l], P.S, P.sr);
      o.key = (l << 16) | b;
      o.r0 = reach_lo(g.sh);
      o.r1 = reach_hi(g.sh + g.bh * (float)P.S);
      o.c0 = reach_lo(g.sw);
      o.c1 = reach_hi(g.sw + g.bw * (float)P.S);
      o.gh = g.gh;
      o.gw = g.gw;
      gv = (f32x4_t){g.sw, g.sh, g.bw, g.bh};
    }
    rec[r] = o;
    geo[r] = gv;
  }
}

template <bool F16>
__global__ __launch_bounds__(ROI_BLK) void roi_align_bwd_kernel(const RoiLevels P, const RoiRec* __restrict__ rec,
                                                                 const f32x4_t* __restrict__ geo, int64_t R,
                                                                 const bf16_t* __restrict__ dout) {
  __shared__ int list[ROI_BLK];
  __shared__ int wave_n[ROI_BLK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int l = 0;
  while (l + 1 < P.L && (int)blockIdx.x >= P.blk_off[l + 1]) ++l;
  int idx = (int)blockIdx.x - P.blk_off[l];
  const int chunk = idx % P.nchunk;
  idx /= P.nchunk;
  const int tx = idx % P.tiles_x[l];
  idx /= P.tiles_x[l];
  const int ty = idx % P.tiles_y[l];
  const int b = idx / P.tiles_y[l];
  const int H = P.H[l], W = P.W[l], S = P.S, C = P.C;
  const float Hf = (float)H, Wf = (float)W;
  const int y = ty * BWD_TH + wave;                      // this wave's pixel row
  const int x0 = tx * BWD_TW + (lane >> 5) * 8;          // this lane's 8 pixel columns
  const int cg = chunk * BWD_CG + (lane & 31);
  const bool cact = cg < P.CG;
  const int key = (l << 16) | b;
  const int ty0 = ty * BWD_TH, tx0 = tx * BWD_TW;
  float acc[8][8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[j][c] = 0.f;

  for (int64_t base = 0; base < R; base += ROI_BLK) {
    const int64_t i = base + tid;
    bool hit = false;
    if (i < R) {
      const RoiRec o = rec[i];
      hit = o.key == key && o.r0 <= ty0 + BWD_TH - 1 && o.r1 >= ty0 && o.c0 <= tx0 + BWD_TW - 1 && o.c1 >= tx0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int off = 0, n = 0;
#pragma unroll
    for (int w = 0; w < ROI_BLK / 64; ++w) {
      off += w < wave ? wave_n[w] : 0;
      n += wave_n[w];
    }
    if (hit) list[off + __popcll(m & ((1ull << lane) - 1ull))] = (int)(i - base);
    __syncthreads();
    for (int e = 0; e < n; ++e) {
      if (y >= H) break;                                 // wave-uniform
      const int64_t r = base + list[e];
      const RoiRec o = rec[r];
      const f32x4_t g = geo[r];
      const int gh = o.gh, gw = o.gw;
      const int ns = gh * gw;
      const float cnt = (float)(ns > 1 ? ns : 1);
      const bf16_t* drow = dout + r * S * S * C + cg * 8;
      for (int ph = 0; ph < S; ++ph) {
        for (int iy = 0; iy < gh; ++iy) {
          const float sy = roi_sample(g[1], ph, g[3], iy, gh);
          if (sy < -1.f || sy > Hf) continue;
          const Axis ay = roi_axis(sy, H);
          if (ay.lo != y && ay.hi != y) continue;        // wave-uniform
          const float wy = __fadd_rn(ay.lo == y ? ay.h : 0.f, ay.hi == y ? ay.l : 0.f);   // lo == hi: l == 0
          for (int pw = 0; pw < S; ++pw) {
            const float xa = __fadd_rn(g[0], __fmul_rn((float)pw, g[2]));
            const float xb = __fadd_rn(xa, g[2]);
            if (xb + 4.f < (float)x0 || xa - 4.f > (float)(x0 + 7) || !cact) continue;   // no corner here
            float gc[8];
            widen8<F16>(*(const s16x8_t*)(drow + (ph * S + pw) * C), gc);
#pragma unroll
            for (int c = 0; c < 8; ++c) gc[c] = __fdiv_rn(gc[c], cnt);
            for (int ix = 0; ix < gw; ++ix) {
              const float sx = roi_sample(g[0], pw, g[2], ix, gw);
              if (sx < -1.f || sx > Wf) continue;
              const Axis ax = roi_axis(sx, W);
              const int dl = ax.lo - x0, dh = ax.hi - x0;
              if ((unsigned)dl >= 8u && (unsigned)dh >= 8u) continue;
              const float wl = __fmul_rn(wy, ax.h), wh = __fmul_rn(wy, ax.l);
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                if (dl == j || dh == j) {
                  const float wj = __fadd_rn(dl == j ? wl : 0.f, dh == j ? wh : 0.f);   // lo == hi: wh == 0
#pragma unroll
                  for (int c = 0; c < 8; ++c) acc[j][c] = __fadd_rn(acc[j][c], __fmul_rn(gc[c], wj));
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();                                     // list is rewritten by the next chunk
  }
  if (y < H && cact) {
    bf16_t* dst = P.ptr[l] + b * P.sn[l] + y * P.sh[l] + cg * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (x0 + j < W) {
        s16x8_t v;
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = __builtin_bit_cast(short, f32_to_elem<F16>(acc[j][c]));
        *(s16x8_t*)(dst + (x0 + j) * P.sw[l]) = v;
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------
static int roi_plan(const char* fn, const tdn_roi_level* lv, int L, int B, int C, const tdn_roi_config* cfg,
                    RoiLevels* P) {
  TDN_CHECK(lv && cfg, "%s: NULL levels / config", fn);
  TDN_CHECK(L >= 1 && L <= TDN_ROI_MAX_LEVELS, "%s: %d levels (1..%d)", fn, L, TDN_ROI_MAX_LEVELS);
  TDN_CHECK(B >= 1 && B <= 65535, "%s: batch size %d (1..65535)", fn, B);
  TDN_CHECK(C >= 8 && C % 8 == 0, "%s: C = %d must be a positive multiple of 8", fn, C);
  TDN_CHECK(cfg->out_size >= 1 && cfg->out_size <= TDN_ROI_MAX_OUT, "%s: out_size %d (1..%d)", fn, cfg->out_size,
            TDN_ROI_MAX_OUT);
  TDN_CHECK(cfg->sampling_ratio >= 0 && cfg->sampling_ratio <= TDN_ROI_MAX_SAMPLES, "%s: sampling_ratio %d (0..%d)",
            fn, cfg->sampling_ratio, TDN_ROI_MAX_SAMPLES);
  TDN_CHECK(cfg->finest_scale > 0.f && cfg->finest_scale < INFINITY, "%s: finest_scale must be positive", fn);
  memset(P, 0, sizeof(*P));
  int64_t blocks = 0;
  const int CG = C / 8, nchunk = (CG + BWD_CG - 1) / BWD_CG;
  for (int l = 0; l < L; ++l) {
    const tdn_roi_level& v = lv[l];
    TDN_CHECK(v.dtype == TDN_BF16 || v.dtype == TDN_F16, "%s: level %d: dtype %d is neither TDN_BF16 nor TDN_F16",
              fn, l, v.dtype);
    TDN_CHECK(v.dtype == lv[0].dtype, "%s: level %d has another dtype than level 0", fn, l);
    TDN_CHECK(v.H >= 1 && v.W >= 1 && v.H < (1 << 20) && v.W < (1 << 20), "%s: level %d: bad H x W %d x %d", fn, l,
              v.H, v.W);
    TDN_CHECK(v.data && ((uintptr_t)v.data & 15) == 0, "%s: level %d: data must be non-NULL and 16-byte aligned", fn,
              l);
    TDN_CHECK(v.strides[1] == 1, "%s: level %d: channel stride %lld, must be 1 (NHWC memory)", fn, l,
              (long long)v.strides[1]);
    TDN_CHECK(v.strides[0] > 0 && v.strides[2] > 0 && v.strides[3] > 0 && v.strides[0] % 8 == 0 &&
                  v.strides[2] % 8 == 0 && v.strides[3] % 8 == 0,
              "%s: level %d: n / h / w strides must be positive multiples of 8", fn, l);
    const float sc = cfg->scales[l];
    TDN_CHECK(sc > 0.f && sc < INFINITY, "%s: level %d: spatial scale must be positive and finite", fn, l);
    P->ptr[l] = (bf16_t*)v.data;
    P->sn[l] = v.strides[0];
    P->sh[l] = v.strides[2];
    P->sw[l] = v.strides[3];
    P->H[l] = v.H;
    P->W[l] = v.W;
    P->scale[l] = sc;
    P->tiles_y[l] = (v.H + BWD_TH - 1) / BWD_TH;
    P->tiles_x[l] = (v.W + BWD_TW - 1) / BWD_TW;
    P->blk_off[l] = (int)blocks;
    blocks += (int64_t)B * P->tiles_y[l] * P->tiles_x[l] * nchunk;
    TDN_CHECK(blocks < (1ll << 31), "%s: too many tiles", fn);
  }
  for (int l = L; l <= TDN_ROI_MAX_LEVELS; ++l) P->blk_off[l] = (int)blocks;
  P->L = L;
  P->B = B;
  P->C = C;
  P->CG = CG;
  P->S = cfg->out_size;
  P->sr = cfg->sampling_ratio;
  P->nchunk = nchunk;
  P->finest = cfg->finest_scale;
  return 0;
}

static int grid_of(int64_t n, int blk) { return tdn_grid_1d(n, blk, 65536); }

extern "C" int tdn_roi_map_levels(const float* rois, int64_t R, int nlevels, float finest_scale, int64_t* levels,
                                  void* stream) {
  TDN_CHECK(R >= 0 && R < (1ll << 31), "tdn_roi_map_levels: bad R");
  TDN_CHECK(nlevels >= 1 && nlevels <= TDN_ROI_MAX_LEVELS, "tdn_roi_map_levels: %d levels (1..%d)", nlevels,
            TDN_ROI_MAX_LEVELS);
  TDN_CHECK(finest_scale > 0.f && finest_scale < INFINITY, "tdn_roi_map_levels: finest_scale must be positive");
  if (R == 0) return 0;
  TDN_CHECK(rois && levels, "tdn_roi_map_levels: NULL pointer");
  TDN_LAUNCH(roi_map_levels_kernel, dim3(grid_of(R, 256)), dim3(256), 0, (hipStream_t)stream, rois, R, nlevels,
             finest_scale, levels);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_roi_align_fwd(const tdn_roi_level* feats, int nlevels, int B, int C, const float* rois, int64_t R,
                                 const tdn_roi_config* cfg, void* out, void* stream) {
  RoiLevels P;
  if (roi_plan("tdn_roi_align_fwd", feats, nlevels, B, C, cfg, &P) != 0) return -1;
  TDN_CHECK(R >= 0 && R < (1ll << 31), "tdn_roi_align_fwd: bad R");
  if (R == 0) return 0;
  TDN_CHECK(rois && out && ((uintptr_t)out & 15) == 0, "tdn_roi_align_fwd: NULL or misaligned rois / out");
  const int64_t total = R * P.S * P.S * P.CG;
  const int dt = feats[0].dtype;
  TDN_LAUNCH_T(roi_align_fwd_kernel, dt, dim3(grid_of(total, ROI_BLK)), dim3(ROI_BLK), stream, P, rois, R,
               (bf16_t*)out);
  TDN_LAUNCH_CHECK();
  return 0;
}

struct RoiBwdWs { RoiRec* rec; f32x4_t* geo; int64_t bytes; };
static RoiBwdWs roi_bwd_layout(int64_t R, void* base) {   // a braced list is evaluated left to right
  const int64_t n = R > 0 ? R : 1;             // R = 0 still launches the gradient kernel
  tdn_carver c{(char*)base, 0};
  return {c.take<RoiRec>(n), c.take<f32x4_t>(n), c.off};
}
extern "C" int64_t tdn_roi_align_bwd_workspace(int64_t R) {
  return (R < 0 || R >= (1ll << 31)) ? -1 : roi_bwd_layout(R, nullptr).bytes;
}

extern "C" int tdn_roi_align_bwd(const tdn_roi_level* grads, int nlevels, int B, int C, const float* rois, int64_t R,
                                 const tdn_roi_config* cfg, const void* dout, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  RoiLevels P;
  if (roi_plan("tdn_roi_align_bwd", grads, nlevels, B, C, cfg, &P) != 0) return -1;
  TDN_CHECK(R >= 0 && R < (1ll << 31), "tdn_roi_align_bwd: bad R");
  TDN_CHECK(R == 0 || (rois && dout && ((uintptr_t)dout & 15) == 0),
            "tdn_roi_align_bwd: NULL or misaligned rois / dout");
  const RoiBwdWs w = roi_bwd_layout(R, workspace);
  if (tdn_check_ws("tdn_roi_align_bwd", workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (R > 0) {
    TDN_LAUNCH(roi_prep_kernel, dim3(grid_of(R, 256)), dim3(256), 0, st, P, rois, R, w.rec, w.geo);
    TDN_LAUNCH_CHECK();
  }
  const int dt = grads[0].dtype;
  TDN_LAUNCH_T(roi_align_bwd_kernel, dt, dim3(P.blk_off[nlevels]), dim3(ROI_BLK), st, P, (const RoiRec*)w.rec,
               (const f32x4_t*)w.geo, R, (const bf16_t*)dout);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_rois_from_proposals(const float* proposals, const int32_t* counts, int B, int M, float* rois,
                                       void* stream) {
  TDN_CHECK(B >= 0 && M >= 0 && (int64_t)B * M < (1ll << 31), "tdn_rois_from_proposals: bad B / M");
  if ((int64_t)B * M == 0) return 0;
  TDN_CHECK(proposals && counts && rois, "tdn_rois_from_proposals: NULL pointer");
  TDN_LAUNCH(rois_from_proposals_kernel, dim3(grid_of((int64_t)B * M, 256)), dim3(256), 0, (hipStream_t)stream,
             proposals, counts, B, M, rois);
  TDN_LAUNCH_CHECK();
  return 0;
}
