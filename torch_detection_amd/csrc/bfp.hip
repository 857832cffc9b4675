// Balanced Feature Pyramid (Libra R-CNN's BFP neck, mmdetection v1) over ALL levels of a pyramid (gfx950), DESIGN.md §4r.
//
//   gather    bsf[q]   = (sum over the levels, ascending, of M_l(x_l)[q]) / L        M_l: adaptive max pool (l < refine level)
//   (refine)  bsf'     = refine(bsf), the caller's conv unit, or bsf itself              or nearest resize (l >= refine level)
//   scatter   out_l[p] = N_l(bsf')[p] + x_l[p]                                       N_l: nearest resize (l < refine level)
//                                                                                        or adaptive max pool (l >= refine level)
// Four launches: gather and scatter forward, and their adjoints.  Both resizing rules are ONE thing here, an axis map
// from a source grid to a destination grid that gives every destination index d a window [lo(d), hi(d)) of the source:
//   pool     lo = floor(d n_src / n_dst), hi = ceil((d + 1) n_src / n_dst)     (torch's adaptive pooling; neighbouring
//                                                                               windows overlap when n_dst does not divide n_src)
//   nearest  lo = min((int)floorf((float)d * scale), n_src - 1), hi = lo + 1,  scale = (float)n_src / (float)n_dst formed on
//                                                                               the host: torch's rule, evaluated in fp32
// and the value of a destination element is the FIRST maximum of its 2-D window in row-major order (strict > against a
// running maximum that starts at the window's first element; a 1 x 1 window is a copy).  Inputs are finite.
// The adjoints are in gather form: a source element s sums, in row-major order of d, the cotangents of the destinations
// d whose window contains s (a contiguous range per axis, because lo and hi never decrease) AND whose first maximum is
// s; that is recomputed from the stored source — s is the first maximum iff every earlier element of the window is
// smaller and no later one is larger — so the forward stores no indices.  Every output element is written by exactly one
// lane, with plain stores: no atomics, no workspace, the same bits on every run.
// All four kernels are memory-bound: a lane owns 8 channels (16 bytes) of one pixel, channels run across the wavefront.
#include "pyramid_core.h"

namespace {

constexpr int MAXL = TDN_PYR_MAX_LEVELS;
constexpr int kThreads = 256;
constexpr int POOL = 0, NEAREST = 1;

struct Axis { int n_src, n_dst, mode; float scale; };
struct Map2 { Axis y, x; };

struct BfpArgs {
  const bf16_t* x[MAXL];      // the level's input (gather, scatter forward: the addend; gather backward: arg-max source)
  const bf16_t* g[MAXL];      // the level's cotangent (backward)
  bf16_t* out[MAXL];          // scatter forward: out_l; gather backward: dx_l
  Map2 gather[MAXL];          // level grid -> refine grid
  Map2 scatter[MAXL];         // refine grid -> level grid
  int H[MAXL], W[MAXL];
  int first_wg[MAXL + 1];     // first workgroup of a level in the per-level launches
  int n, B, C8, Hg, Wg;
  float num_levels;           // the divisor L, as the float it is divided by
};

__device__ __forceinline__ int win_lo(const Axis& a, int d) {
  if (a.mode == POOL) return (int)(((int64_t)d * a.n_src) / a.n_dst);
  const int s = (int)floorf(__fmul_rn((float)d, a.scale));
  return s < a.n_src - 1 ? s : a.n_src - 1;
}
__device__ __forceinline__ int win_hi(const Axis& a, int d, int lo) {
  if (a.mode == POOL) return (int)((((int64_t)d + 1) * a.n_src + a.n_dst - 1) / a.n_dst);
  return lo + 1;
}

// the destinations whose window contains source index s: [dlo, dhi), possibly empty for a nearest map
__device__ __forceinline__ void cover(const Axis& a, int s, int& dlo, int& dhi) {
  if (a.mode == POOL) {
    dlo = (int)(((int64_t)s * a.n_dst) / a.n_src);
    dhi = (int)((((int64_t)s + 1) * a.n_dst + a.n_src - 1) / a.n_src);
    return;
  }
  // nearest: the source index never decreases with d; the first d that reaches s, and the first that reaches s + 1
  int lo = 0, hi = a.n_dst;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (win_lo(a, mid) >= s) hi = mid; else lo = mid + 1;
  }
  dlo = lo;
  hi = a.n_dst;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (win_lo(a, mid) >= s + 1) hi = mid; else lo = mid + 1;
  }
  dhi = lo;
}

template <bool F16>
__device__ __forceinline__ void load8(const bf16_t* p, float* v) {
  const bf16x8_t r = *(const bf16x8_t*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = elem_to_f32<F16>(r[e]);
}
template <bool F16>
__device__ __forceinline__ void store8(bf16_t* p, const float* v) {
  bf16x8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f32_to_elem<F16>(v[e]);
  *(bf16x8_t*)p = o;
}

// first maximum of destination (dy, dx)'s window of `src`, an image (n_src_y, n_src_x, C) whose lane base is given
template <bool F16>
__device__ __forceinline__ void window_max(const Map2& m, const bf16_t* src, int64_t pitch, int dy, int dx, float* v) {
  const int y0 = win_lo(m.y, dy), y1 = win_hi(m.y, dy, y0);
  const int x0 = win_lo(m.x, dx), x1 = win_hi(m.x, dx, x0);
  load8<F16>(src + ((int64_t)y0 * m.x.n_src + x0) * pitch, v);
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) {
      if (yy == y0 && xx == x0) continue;
      float t[8];
      load8<F16>(src + ((int64_t)yy * m.x.n_src + xx) * pitch, t);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = t[e] > v[e] ? t[e] : v[e];
    }
}

// acc += the adjoint of map m at source element (sy, sx): the cotangents `cot` (an image (n_dst_y, n_dst_x, C)) of the
// destinations whose window contains the element and has its first maximum there, in row-major order
template <bool F16>
__device__ __forceinline__ void adjoint_sum(const Map2& m, const bf16_t* src, const bf16_t* cot, int64_t pitch, int sy,
                                            int sx, float* acc) {
  int dy0, dy1, dx0, dx1;
  cover(m.y, sy, dy0, dy1);
  cover(m.x, sx, dx0, dx1);
  if (dy0 >= dy1 || dx0 >= dx1) return;
  float me[8];
  load8<F16>(src + ((int64_t)sy * m.x.n_src + sx) * pitch, me);
  for (int dy = dy0; dy < dy1; ++dy) {
    const int y0 = win_lo(m.y, dy), y1 = win_hi(m.y, dy, y0);
    for (int dx = dx0; dx < dx1; ++dx) {
      const int x0 = win_lo(m.x, dx), x1 = win_hi(m.x, dx, x0);
      bool mine[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) mine[e] = true;
      for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
          if (yy == sy && xx == sx) continue;
          const bool before = yy < sy || (yy == sy && xx < sx);
          float t[8];
          load8<F16>(src + ((int64_t)yy * m.x.n_src + xx) * pitch, t);
#pragma unroll
          for (int e = 0; e < 8; ++e) mine[e] = mine[e] && (before ? t[e] < me[e] : t[e] <= me[e]);
        }
      float gv[8];
      load8<F16>(cot + ((int64_t)dy * m.x.n_dst + dx) * pitch, gv);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = mine[e] ? __fadd_rn(acc[e], gv[e]) : acc[e];
    }
  }
}

// lane i of an image batch (B, H, W, C8 lanes): -> image, row, column, channel lane
struct LaneAt { int b, y, x, c; };
__device__ __forceinline__ LaneAt lane_at(int i, int W, int HW, int C8) {
  const int pix = i / C8;
  LaneAt a;
  a.c = i - pix * C8;
  a.b = pix / HW;
  const int r = pix - a.b * HW;
  a.y = r / W;
  a.x = r - a.y * W;
  return a;
}

// [1] bsf[q] = (0 + M_0(x_0)[q] + M_1(x_1)[q] + ...) / L
template <bool F16>
__global__ __launch_bounds__(kThreads) void bfp_gather_fwd_kernel(const BfpArgs p, bf16_t* __restrict__ bsf) {
  const int HWg = p.Hg * p.Wg;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= p.B * HWg * p.C8) return;
  const LaneAt at = lane_at(i, p.Wg, HWg, p.C8);
  const int64_t pitch = (int64_t)p.C8 * 8;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int l = 0; l < p.n; ++l) {
    float v[8];
    window_max<F16>(p.gather[l], p.x[l] + (int64_t)at.b * p.H[l] * p.W[l] * pitch + at.c * 8, pitch, at.y, at.x, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = __fadd_rn(acc[e], v[e]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = __fdiv_rn(acc[e], p.num_levels);
  store8<F16>(bsf + (int64_t)i * 8, acc);
}

// [2] out_l[p] = N_l(bsf')[p] + x_l[p], all levels
template <bool F16>
__global__ __launch_bounds__(kThreads) void bfp_scatter_fwd_kernel(const BfpArgs p, const bf16_t* __restrict__ bsf) {
  const int l = find_level(p.first_wg, p.n, (int)blockIdx.x);
  const int HW = p.H[l] * p.W[l];
  const int i = ((int)blockIdx.x - p.first_wg[l]) * kThreads + (int)threadIdx.x;
  if (i >= p.B * HW * p.C8) return;
  const LaneAt at = lane_at(i, p.W[l], HW, p.C8);
  const int64_t pitch = (int64_t)p.C8 * 8;
  float v[8], xv[8];
  window_max<F16>(p.scatter[l], bsf + (int64_t)at.b * p.Hg * p.Wg * pitch + at.c * 8, pitch, at.y, at.x, v);
  load8<F16>(p.x[l] + (int64_t)i * 8, xv);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = __fadd_rn(v[e], xv[e]);
  store8<F16>(p.out[l] + (int64_t)i * 8, v);
}

// [3] d bsf'[q] = 0 + s_0 + s_1 + ..., s_l = the adjoint of N_l at q of the level's cotangent, a sum of its own from 0
template <bool F16>
__global__ __launch_bounds__(kThreads) void bfp_scatter_bwd_kernel(const BfpArgs p, const bf16_t* __restrict__ bsf,
                                                                   bf16_t* __restrict__ dbsf) {
  const int HWg = p.Hg * p.Wg;
  const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= p.B * HWg * p.C8) return;
  const LaneAt at = lane_at(i, p.Wg, HWg, p.C8);
  const int64_t pitch = (int64_t)p.C8 * 8;
  const bf16_t* src = bsf + (int64_t)at.b * HWg * pitch + at.c * 8;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int l = 0; l < p.n; ++l) {
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    adjoint_sum<F16>(p.scatter[l], src, p.g[l] + (int64_t)at.b * p.H[l] * p.W[l] * pitch + at.c * 8, pitch, at.y, at.x, s);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = __fadd_rn(acc[e], s[e]);
  }
  store8<F16>(dbsf + (int64_t)i * 8, acc);
}

// [4] dx_l[p] = g_l[p] + s / L, s = the adjoint of M_l at p of d bsf, all levels
template <bool F16>
__global__ __launch_bounds__(kThreads) void bfp_gather_bwd_kernel(const BfpArgs p, const bf16_t* __restrict__ dbsf) {
  const int l = find_level(p.first_wg, p.n, (int)blockIdx.x);
  const int HW = p.H[l] * p.W[l];
  const int i = ((int)blockIdx.x - p.first_wg[l]) * kThreads + (int)threadIdx.x;
  if (i >= p.B * HW * p.C8) return;
  const LaneAt at = lane_at(i, p.W[l], HW, p.C8);
  const int64_t pitch = (int64_t)p.C8 * 8;
  float s[8], gv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  adjoint_sum<F16>(p.gather[l], p.x[l] + (int64_t)at.b * HW * pitch + at.c * 8,
                   dbsf + (int64_t)at.b * p.Hg * p.Wg * pitch + at.c * 8, pitch, at.y, at.x, s);
  load8<F16>(p.g[l] + (int64_t)i * 8, gv);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = __fadd_rn(gv[e], __fdiv_rn(s[e], p.num_levels));
  store8<F16>(p.out[l] + (int64_t)i * 8, s);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
Axis axis_of(int mode, int n_src, int n_dst) {
  return Axis{n_src, n_dst, mode, mode == NEAREST ? (float)n_src / (float)n_dst : 0.f};
}

// what: bit 0 x, bit 1 out, bit 2 g, bit 3 dx are needed
int fill_args(const char* who, const tdn_bfp_level* levels, int n, int refine, int B, int C, int what, BfpArgs& p) {
  TDN_CHECK(levels, "%s: NULL levels", who);
  if (check_levels(who, n, MAXL) != 0) return -1;
  TDN_CHECK(refine >= 0 && refine < n, "%s: refine_level=%d out of 0..%d", who, refine, n - 1);
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(C >= 8 && C <= 1024 && C % 8 == 0, "%s: C=%d is not a multiple of 8 in 8..1024", who, C);
  p = BfpArgs{};
  int64_t lanes[MAXL];
  for (int l = 0; l < n; ++l) {
    const tdn_bfp_level& L = levels[l];
    TDN_CHECK(L.H >= 1 && L.W >= 1 && L.H <= 32767 && L.W <= 32767, "%s: level %d: H=%d, W=%d out of 1..32767", who, l,
              L.H, L.W);
    TDN_CHECK((int64_t)B * L.H * L.W * C < ((int64_t)1 << 31), "%s: level %d holds 2^31 elements or more", who, l);
    TDN_CHECK(!(what & 1) || (L.x && aligned(L.x, 16)), "%s: level %d: x must be a 16-byte aligned pointer", who, l);
    TDN_CHECK(!(what & 2) || (L.out && aligned(L.out, 16)), "%s: level %d: out must be a 16-byte aligned pointer", who, l);
    TDN_CHECK(!(what & 4) || (L.g && aligned(L.g, 16)), "%s: level %d: g must be a 16-byte aligned pointer", who, l);
    TDN_CHECK(!(what & 8) || (L.dx && aligned(L.dx, 16)), "%s: level %d: dx must be a 16-byte aligned pointer", who, l);
    p.x[l] = (const bf16_t*)L.x;
    p.g[l] = (const bf16_t*)L.g;
    p.out[l] = (bf16_t*)((what & 8) ? L.dx : L.out);
    p.H[l] = L.H;
    p.W[l] = L.W;
    lanes[l] = (int64_t)B * L.H * L.W * (C / 8);
  }
  const int64_t wg = fill_first(lanes, n, kThreads, p.first_wg, MAXL);
  TDN_CHECK(wg < ((int64_t)1 << 31), "%s: the pyramid needs 2^31 workgroups or more", who);
  p.n = n; p.B = B; p.C8 = C / 8;
  p.Hg = levels[refine].H; p.Wg = levels[refine].W;
  p.num_levels = (float)n;
  for (int l = 0; l < n; ++l) {
    const int down = l < refine ? POOL : NEAREST, up = l < refine ? NEAREST : POOL;
    p.gather[l] = Map2{axis_of(down, p.H[l], p.Hg), axis_of(down, p.W[l], p.Wg)};
    p.scatter[l] = Map2{axis_of(up, p.Hg, p.H[l]), axis_of(up, p.Wg, p.W[l])};
  }
  return 0;
}

int grid_g(const BfpArgs& p) { return (int)(((int64_t)p.B * p.Hg * p.Wg * p.C8 + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int tdn_bfp_gather_fwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C, void* bsf,
                                  int dtype, void* stream) {
  const char* who = "tdn_bfp_gather_fwd";
  TDN_CHECK_DTYPE(dtype);
  BfpArgs p;
  if (fill_args(who, levels, num_levels, refine_level, B, C, 1, p) != 0) return -1;
  TDN_CHECK(bsf && aligned(bsf, 16), "%s: bsf must be a 16-byte aligned pointer", who);
  TDN_LAUNCH_T(bfp_gather_fwd_kernel, dtype, dim3(grid_g(p)), dim3(kThreads), stream, p, (bf16_t*)bsf);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_bfp_scatter_fwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C,
                                   const void* bsf, int dtype, void* stream) {
  const char* who = "tdn_bfp_scatter_fwd";
  TDN_CHECK_DTYPE(dtype);
  BfpArgs p;
  if (fill_args(who, levels, num_levels, refine_level, B, C, 1 | 2, p) != 0) return -1;
  TDN_CHECK(bsf && aligned(bsf, 16), "%s: bsf must be a 16-byte aligned pointer", who);
  TDN_LAUNCH_T(bfp_scatter_fwd_kernel, dtype, dim3(p.first_wg[MAXL]), dim3(kThreads), stream, p, (const bf16_t*)bsf);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_bfp_scatter_bwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C,
                                   const void* bsf, void* dbsf, int dtype, void* stream) {
  const char* who = "tdn_bfp_scatter_bwd";
  TDN_CHECK_DTYPE(dtype);
  BfpArgs p;
  if (fill_args(who, levels, num_levels, refine_level, B, C, 4, p) != 0) return -1;
  TDN_CHECK(bsf && aligned(bsf, 16) && dbsf && aligned(dbsf, 16), "%s: bsf and dbsf must be 16-byte aligned pointers", who);
  TDN_LAUNCH_T(bfp_scatter_bwd_kernel, dtype, dim3(grid_g(p)), dim3(kThreads), stream, p, (const bf16_t*)bsf,
               (bf16_t*)dbsf);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_bfp_gather_bwd(const tdn_bfp_level* levels, int num_levels, int refine_level, int B, int C,
                                  const void* dbsf, int dtype, void* stream) {
  const char* who = "tdn_bfp_gather_bwd";
  TDN_CHECK_DTYPE(dtype);
  BfpArgs p;
  if (fill_args(who, levels, num_levels, refine_level, B, C, 1 | 4 | 8, p) != 0) return -1;
  TDN_CHECK(dbsf && aligned(dbsf, 16), "%s: dbsf must be a 16-byte aligned pointer", who);
  TDN_LAUNCH_T(bfp_gather_bwd_kernel, dtype, dim3(p.first_wg[MAXL]), dim3(kThreads), stream, p, (const bf16_t*)dbsf);
  TDN_LAUNCH_CHECK();
  return 0;
}
