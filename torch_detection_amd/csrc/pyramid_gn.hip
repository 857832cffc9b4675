// GroupNorm (+ ReLU) with shared affine parameters over ALL levels of a pyramid (gfx950), DESIGN.md §4o.
//
// The tower layers of a single-stage head with norm_cfg GN (mmdetection-v1 FCOSHead: conv -> GroupNorm(32) -> ReLU, the
// same modules on every level) normalise five maps of very different sizes with one (gamma, beta).  Level by level that
// is gn.hip's three launches per map and, in the backward, a mask launch in front of them; here a level table travels in
// the kernel arguments, as in pyramid_conv.hip, and the whole pyramid is three launches each way:
//   forward   [1] per-channel partial (sum d, sum d^2), d = z - K, over the pixel chunks of every (level, image)
//             [2] per (level, image, group) mean / rstd in double -> stats (mu, rstd) and the affine (a, b', K)
//             [3] y = relu?((z - K) * a + b')
//   backward  [1'] per-channel partial (sum g, sum g * xhat), g counted as 0 where y <= 0 (relu), xhat = (z - mu) * rstd
//             [2'] per (level, image): the channel sums (s1, s2) and the coefficients of dz
//             [3'] dz = g * A - xhat * Bq - Cq;  its block 0 also adds the (s1, s2) of all levels and images, level order
//                  finest first, image order within a level, into dgamma / dbeta
// The statistics are norm_core.h's, shared with gn.hip ("Numerics of the statistics"): sums about the pivot
// K_c = the channel's value at pixel 0 of the (level, image), pivots put back in double, output formed about the pivot.
// The chunk cut of a (level, image) is that header's cut_of for the level alone, a function of (B, H_l W_l, C) only: a
// level gives the same bits launched alone, inside a pyramid, or through gn.hip.  Partials are plain stores; every
// reduction runs in a fixed order; no atomics, no counters, no memset.  All passes are HBM-bound, 16 bytes per lane.
#include "norm_core.h"
#include "pyramid_core.h"

namespace {

constexpr int MAXL = TDN_PYR_MAX_LEVELS;
constexpr int TILE = 4 * kThreads;      // 16-byte lanes per workgroup of the apply launches
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;

struct PgnArgs {
  const bf16_t* z[MAXL];
  const bf16_t* g[MAXL];              // backward: the unmasked cotangent
  const bf16_t* y[MAXL];              // backward: the ReLU mask source
  bf16_t* out[MAXL];                  // forward: y; backward: dz
  int HW[MAXL];
  int chunks[MAXL], chunk_px[MAXL];   // pixel chunks per image, pixels per chunk
  int first_wg[MAXL + 1];             // first workgroup of a level in the partial launch (B * chunks each)
  int first_tile[MAXL + 1];           // first workgroup of a level in the apply launch
  int n, B, C, C8, cpg, ppp, relu;
};

// [1] / [1']: partial per-channel sums over one pixel chunk of one (level, image); part layout [workgroup][2][C]
//   MODE 0: (sum d, sum d^2), d = z - K, K = z at pixel 0 of the (level, image)
//   MODE 1: (sum g, sum g * xhat), g taken as 0 where y <= 0 when p.relu
template <int MODE, bool F16>
__global__ __launch_bounds__(kThreads) void pgn_partial_kernel(const PgnArgs p, const float* __restrict__ stats,
                                                                float* __restrict__ part) {
  __shared__ float red[kThreads][17];
  const int l = find_level(p.first_wg, p.n, (int)blockIdx.x);
  const int idx = (int)blockIdx.x - p.first_wg[l];
  const int chunks = p.chunks[l], HW = p.HW[l], C = p.C;
  const int n = idx / chunks, chunk = idx - n * chunks;
  const int tid = threadIdx.x;
  const int cl = tid % p.C8, pl = tid / p.C8;
  const int p0 = chunk * p.chunk_px[l];
  const int p1 = min(HW, p0 + p.chunk_px[l]);
  const bf16_t* __restrict__ z = p.z[l];
  const bf16_t* __restrict__ g = p.g[l];
  const bf16_t* __restrict__ ym = p.y[l];
  float a0[8], a1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
  const int64_t base = (int64_t)n * HW * C + cl * 8;
  float mu[8], rs[8], piv[8];
  if (MODE == 1) {
    const float* s = stats + (((int64_t)l * p.B + n) * C + cl * 8) * 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = s[2 * e]; rs[e] = s[2 * e + 1]; }
  } else {
    const bf16x8_t kv = *(const bf16x8_t*)(z + base);
#pragma unroll
    for (int e = 0; e < 8; ++e) piv[e] = elem_to_f32<F16>(kv[e]);
  }
  const bool relu = p.relu != 0;
  for (int px = p0 + pl; px < p1; px += p.ppp) {
    const bf16x8_t zv = *(const bf16x8_t*)(z + base + (int64_t)px * C);
    if (MODE == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = elem_to_f32<F16>(zv[e]) - piv[e];
        a0[e] += d;
        a1[e] += d * d;
      }
    } else {
      const bf16x8_t gv = *(const bf16x8_t*)(g + base + (int64_t)px * C);
      bf16x8_t yv = gv;
      if (relu) yv = *(const bf16x8_t*)(ym + base + (int64_t)px * C);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float gg = elem_to_f32<F16>(gv[e]);
        if (relu && !(elem_to_f32<F16>(yv[e]) > 0.f)) gg = 0.f;
        const float xh = (elem_to_f32<F16>(zv[e]) - mu[e]) * rs[e];
        a0[e] += gg;
        a1[e] += gg * xh;
      }
    }
  }
  // combine the pixel lanes in lane order (fixed order -> deterministic)
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[tid][e] = a0[e]; red[tid][8 + e] = a1[e]; }
  __syncthreads();
  if (pl == 0) {
    for (int j = 1; j < p.ppp; ++j) {
#pragma unroll
      for (int e = 0; e < 16; ++e) red[tid][e] += red[j * p.C8 + cl][e];
    }
    float* o = part + (int64_t)blockIdx.x * 2 * C + cl * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { o[e] = red[tid][e]; o[C + e] = red[tid][8 + e]; }
  }
}

// [2]: block (channel block of CB = max(32, cpg) channels — whole groups —, level * B + image): norm_core.h's
// group_moments of the channels' (s_c, q_c, K_c).  stats[level][image][c] = (mu, rstd); coef[level][image][3][C] =
// a, b', K of y = (z - K) * a + b' (fwd_coef).
__global__ __launch_bounds__(kThreads) void pgn_stats_kernel(const PgnArgs p, int CB, int f16,
                                                             const float* __restrict__ part,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             float* __restrict__ stats, float* __restrict__ coef) {
  __shared__ double red[2 * kThreads];
  __shared__ double tot[3 * kThreads];
  const int l = (int)blockIdx.y / p.B, n = (int)blockIdx.y - l * p.B;
  const int HW = p.HW[l], C = p.C;
  const int KL = kThreads / CB;
  const int cl = threadIdx.x % CB, kl = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cl;                    // < C: CB divides C
  if (HW == 0) {                                         // the whole block: an empty level has nothing to read;
    if (kl == 0) {                                       // its rows of stats are zero, so that all of stats is defined
      float* o = stats + (((int64_t)l * p.B + n) * C + c) * 2;
      o[0] = 0.f;
      o[1] = 0.f;
    }
    return;
  }
  const bf16_t* z = p.z[l] + (int64_t)n * HW * C + c;
  const double K = kl == 0 ? pivot_of(z, f16) : 0.0;     // asked for ahead of the chunk sums: its latency hides
  double s, ss;
  row_totals(part + ((int64_t)p.first_wg[l] + (int64_t)n * p.chunks[l]) * 2 * C, p.chunks[l], C, c, cl, kl, CB, KL, red,
             s, ss);
  if (kl == 0) { tot[cl] = s; tot[kThreads + cl] = ss; tot[2 * kThreads + cl] = K; }
  __syncthreads();
  if (kl == 0) {
    const Moments m = group_moments(tot, (cl / p.cpg) * p.cpg, p.cpg, HW, eps);
    const int64_t row = (int64_t)l * p.B + n;
    stats[(row * C + c) * 2] = (float)m.mu;
    stats[(row * C + c) * 2 + 1] = m.rstd;
    float a, b;
    fwd_coef(m.rstd, gamma[c], beta[c], m.mu - K, a, b);
    float* o = coef + row * 3 * C + c;
    o[0] = a;
    o[C] = b;
    o[2 * C] = (float)K;
  }
}

// the (image, channel lane) of 16-byte lane i of a level, i = base + j with base the tile's first lane
struct LaneAt { int n, cl; };
__device__ __forceinline__ LaneAt lane_at(int64_t n0, int64_t r0, int j, int64_t per_n, int C8) {
  const int64_t q = r0 + j;                              // < per_n + TILE
  int n;
  if (per_n <= 0x7fffffff) n = (int)n0 + (int)((uint32_t)q / (uint32_t)per_n);
  else n = (int)n0 + (q >= per_n ? 1 : 0);
  return LaneAt{n, (int)(q & (C8 - 1))};                 // per_n is a multiple of C8, C8 a power of two
}

// [3]: y = relu?((z - K) * a + b'), one tile of TILE 16-byte lanes of one level per workgroup
template <bool F16>
__global__ __launch_bounds__(kThreads) void pgn_apply_kernel(const PgnArgs p, const float* __restrict__ coef) {
  const int l = find_level(p.first_tile, p.n, (int)blockIdx.x);
  const int C = p.C;
  const int64_t per_n = (int64_t)p.HW[l] * p.C8, total = per_n * p.B;
  const int64_t base = (int64_t)((int)blockIdx.x - p.first_tile[l]) * TILE;
  const int64_t n0 = base / per_n, r0 = base - n0 * per_n;
  const bf16_t* __restrict__ z = p.z[l];
  bf16_t* __restrict__ y = p.out[l];
  const bool relu = p.relu != 0;
  bf16x8_t zv[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t i = base + it * kThreads + threadIdx.x;
    if (i < total) zv[it] = *(const bf16x8_t*)(z + i * 8);
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = it * kThreads + threadIdx.x;
    const int64_t i = base + j;
    if (i >= total) continue;
    const LaneAt at = lane_at(n0, r0, j, per_n, p.C8);
    const float* cf = coef + ((int64_t)l * p.B + at.n) * 3 * C + at.cl * 8;
    bf16x8_t o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4_t ca = *(const f32x4_t*)(cf + 4 * h), cb = *(const f32x4_t*)(cf + C + 4 * h);
      const f32x4_t ck = *(const f32x4_t*)(cf + 2 * C + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = (elem_to_f32<F16>(zv[it][4 * h + e]) - ck[e]) * ca[e] + cb[e];
        o[4 * h + e] = f32_to_elem<F16>(relu ? fmaxf(v, 0.f) : v);
      }
    }
    *(bf16x8_t*)(y + i * 8) = o;
  }
}

// [2']: block (channel block, level * B + image): chunk sums -> (s1, s2) = (sum g, sum g xhat) of every channel, kept in
// sums[level][image][2][C] for the level-ordered total of [3'], and the group means m1 = sum_c gamma s1 / cnt,
// m2 = sum_c gamma s2 / cnt.  coef[level][image][3][C] = A, Bq, Cq of dz = g A - xhat Bq - Cq:
//   A = rstd gamma, Bq = rstd m2, Cq = rstd m1     (dz = rstd (gamma g - m1 - xhat m2))
__global__ __launch_bounds__(kThreads) void pgn_bwd_coef_kernel(const PgnArgs p, int CB, const float* __restrict__ part,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ stats,
                                                                float* __restrict__ coef, float* __restrict__ sums) {
  __shared__ double red[2 * kThreads];
  __shared__ float t1[kThreads], t2[kThreads];
  const int l = (int)blockIdx.y / p.B, n = (int)blockIdx.y - l * p.B;
  const int HW = p.HW[l], C = p.C;
  if (HW == 0) return;
  const int KL = kThreads / CB;
  const int cl = threadIdx.x % CB, kl = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cl;
  const float gm = gamma[c];
  double d1, d2;
  row_totals(part + ((int64_t)p.first_wg[l] + (int64_t)n * p.chunks[l]) * 2 * C, p.chunks[l], C, c, cl, kl, CB, KL, red,
             d1, d2);
  const float s1 = (float)d1, s2 = (float)d2;
  if (kl == 0) { t1[cl] = gm * s1; t2[cl] = gm * s2; }
  __syncthreads();
  if (kl == 0) {
    float m1, m2;
    group_means(t1, t2, (cl / p.cpg) * p.cpg, p.cpg, (float)HW * (float)p.cpg, m1, m2);
    const int64_t row = (int64_t)l * p.B + n;
    const float r = stats[(row * C + c) * 2 + 1];
    float* o = coef + row * 3 * C + c;
    o[0] = r * gm;
    o[C] = r * m2;
    o[2 * C] = r * m1;
    sums[row * 2 * C + c] = s1;
    sums[row * 2 * C + C + c] = s2;
  }
}

// [3']: dz = g A - xhat Bq - Cq with g taken as 0 where y <= 0 (relu), xhat = (z - mu) rstd; block 0 first adds the
// channel sums of all (level, image) pairs in table order into dgamma / dbeta (acc: 0 overwrites, else acc * old + sum).
// `tiles` workgroups have a tile; the grid is max(tiles, 1) so that the totals are written for an empty pyramid too.
template <bool F16>
__global__ __launch_bounds__(kThreads) void pgn_bwd_apply_kernel(const PgnArgs p, int tiles,
                                                                 const float* __restrict__ coef,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ sums, float* dgamma,
                                                                 float* dbeta, float acc) {
  const int C = p.C;
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += kThreads) {
      float dg = 0.f, db = 0.f;
      for (int l = 0; l < p.n; ++l) {
        if (p.HW[l] == 0) continue;
        for (int n = 0; n < p.B; ++n) {
          const float* s = sums + ((int64_t)l * p.B + n) * 2 * C + c;
          db += s[0];
          dg += s[C];
        }
      }
      dgamma[c] = (acc != 0.f) ? acc * dgamma[c] + dg : dg;
      dbeta[c] = (acc != 0.f) ? acc * dbeta[c] + db : db;
    }
  }
  if ((int)blockIdx.x >= tiles) return;
  const int l = find_level(p.first_tile, p.n, (int)blockIdx.x);
  const int64_t per_n = (int64_t)p.HW[l] * p.C8, total = per_n * p.B;
  const int64_t base = (int64_t)((int)blockIdx.x - p.first_tile[l]) * TILE;
  const int64_t n0 = base / per_n, r0 = base - n0 * per_n;
  const bf16_t* __restrict__ z = p.z[l];
  const bf16_t* __restrict__ g = p.g[l];
  const bf16_t* __restrict__ ym = p.y[l];
  bf16_t* __restrict__ dz = p.out[l];
  const bool relu = p.relu != 0;
  bf16x8_t zv[4], gv[4], yv[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t i = base + it * kThreads + threadIdx.x;
    if (i < total) {
      zv[it] = *(const bf16x8_t*)(z + i * 8);
      gv[it] = *(const bf16x8_t*)(g + i * 8);
      yv[it] = relu ? *(const bf16x8_t*)(ym + i * 8) : gv[it];
    }
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = it * kThreads + threadIdx.x;
    const int64_t i = base + j;
    if (i >= total) continue;
    const LaneAt at = lane_at(n0, r0, j, per_n, p.C8);
    const int64_t row = (int64_t)l * p.B + at.n;
    const float* cf = coef + row * 3 * C + at.cl * 8;
    const float* st = stats + (row * C + at.cl * 8) * 2;
    bf16x8_t o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4_t ca = *(const f32x4_t*)(cf + 4 * h), cb = *(const f32x4_t*)(cf + C + 4 * h);
      const f32x4_t cc = *(const f32x4_t*)(cf + 2 * C + 4 * h);
      const f32x4_t s0 = *(const f32x4_t*)(st + 8 * h), s1 = *(const f32x4_t*)(st + 8 * h + 4);
      const float mu[4] = {s0[0], s0[2], s1[0], s1[2]}, rs[4] = {s0[1], s0[3], s1[1], s1[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gg = elem_to_f32<F16>(gv[it][4 * h + e]);
        if (relu && !(elem_to_f32<F16>(yv[it][4 * h + e]) > 0.f)) gg = 0.f;
        const float xh = (elem_to_f32<F16>(zv[it][4 * h + e]) - mu[e]) * rs[e];
        o[4 * h + e] = f32_to_elem<F16>(gg * ca[e] - xh * cb[e] - cc[e]);
      }
    }
    *(bf16x8_t*)(dz + i * 8) = o;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct PgnPlan {
  int C8, cpg, ppp, CB;
  int HW[MAXL], chunks[MAXL], chunk_px[MAXL];
  int first_wg[MAXL + 1], first_tile[MAXL + 1];
  int wgs, tiles, live;               // workgroups of the partial launch, of the apply launch; levels with pixels
};

int check_shape(const char* who, int kind, int B, const int32_t* hw, int n, int C, int G) {
  TDN_CHECK(kind == 0 || kind == 1, "%s: kind %d is neither 0 (forward) nor 1 (backward)", who, kind);
  if (check_levels(who, n, MAXL) != 0) return -1;
  TDN_CHECK(hw, "%s: NULL level sizes", who);
  TDN_CHECK(B >= 0 && B <= 65535 / MAXL, "%s: B=%d out of 0..%d", who, B, 65535 / MAXL);
  TDN_CHECK(C == 64 || C == 128 || C == 256 || C == 512, "%s: C=%d is none of 64, 128, 256, 512", who, C);
  TDN_CHECK(G > 0 && C % G == 0, "%s: %d groups do not divide %d channels", who, G, C);
  TDN_CHECK(C / G <= 256, "%s: %d channels per group not supported (at most 256)", who, C / G);
  int64_t wgs = 0, tiles = 0;
  for (int l = 0; l < n; ++l) {
    const int64_t H = hw[2 * l], W = hw[2 * l + 1];
    TDN_CHECK(H >= 0 && W >= 0, "%s: level %d: H=%lld, W=%lld must not be negative", who, l, (long long)H, (long long)W);
    TDN_CHECK(H * W < MAX_ROWS && (int64_t)B * H * W < MAX_ROWS, "%s: level %d: B*H*W out of 0..2^31-1", who, l);
    wgs += (int64_t)B * 1024;                                    // an upper bound of B * chunks
    tiles += ((int64_t)B * H * W * (C / 8) + TILE - 1) / TILE;
  }
  TDN_CHECK(wgs < MAX_ROWS && tiles < MAX_ROWS, "%s: the pyramid needs more than 2^31 - 1 workgroups", who);
  return 0;
}

// The cut of level l is norm_core.h's cut_of for a map of its size alone: a function of (B, H_l * W_l, C).
void make_plan(int B, const int32_t* hw, int n, int C, int G, PgnPlan& pl) {
  pl.C8 = C / 8;
  pl.cpg = C / G;
  pl.ppp = pixel_lanes(pl.C8);
  pl.CB = pl.cpg > 32 ? pl.cpg : 32;
  int wg = 0;
  int64_t lanes[MAXL] = {};
  pl.live = 0;
  for (int l = 0; l < MAXL; ++l) {
    pl.first_wg[l] = wg;
    pl.HW[l] = pl.chunks[l] = pl.chunk_px[l] = 0;
    if (l >= n) continue;
    const int HW = B > 0 ? hw[2 * l] * hw[2 * l + 1] : 0;
    if (HW == 0) continue;
    const Cut cut = cut_of(B, HW, pl.C8);
    pl.HW[l] = HW;
    pl.chunk_px[l] = cut.chunk_px;
    pl.chunks[l] = cut.chunks;
    wg += B * pl.chunks[l];
    lanes[l] = (int64_t)B * HW * pl.C8;
    ++pl.live;
  }
  pl.first_wg[MAXL] = wg;
  pl.wgs = wg;
  pl.tiles = (int)fill_first(lanes, n, TILE, pl.first_tile, MAXL);
}

// workspace: part [workgroup][2][C] | coef [level][B][3][C] | backward only: sums [level][B][2][C]
struct PgnWs { float* part; float* coef; float* sums; int64_t bytes; };
PgnWs ws_layout(int kind, const PgnPlan& pl, int n, int B, int C, void* base) {
  tdn_carver c{(char*)base, 0};
  PgnWs w{nullptr, nullptr, nullptr, 0};
  if (pl.wgs > 0) {
    w.part = c.take<float>((int64_t)pl.wgs * 2 * C);
    w.coef = c.take<float>((int64_t)n * B * 3 * C);
    if (kind == 1) w.sums = c.take<float>((int64_t)n * B * 2 * C);
  }
  w.bytes = c.off;
  return w;
}

int fill_args(const char* who, int kind, const tdn_pyr_gn_level* levels, int n, int B, int C, int relu,
              const PgnPlan& pl, PgnArgs& p) {
  p = PgnArgs{};
  for (int l = 0; l < n; ++l) {
    if (pl.HW[l] == 0) continue;                         // skipped: its pointers are not looked at
    const tdn_pyr_gn_level& L = levels[l];
    TDN_CHECK(L.z && aligned(L.z, 16), "%s: level %d: z must be a 16-byte aligned pointer", who, l);
    if (kind == 0) {
      TDN_CHECK(L.y && aligned(L.y, 16), "%s: level %d: y must be a 16-byte aligned pointer", who, l);
      p.out[l] = (bf16_t*)L.y;
    } else {
      TDN_CHECK(L.g && aligned(L.g, 16) && L.dz && aligned(L.dz, 16), "%s: level %d: g and dz must be 16-byte aligned pointers",
                who, l);
      TDN_CHECK(!relu || (L.y && aligned(L.y, 16)), "%s: level %d: y (the ReLU mask source) must be a 16-byte aligned pointer",
                who, l);
      p.g[l] = (const bf16_t*)L.g;
      p.y[l] = (const bf16_t*)L.y;
      p.out[l] = (bf16_t*)L.dz;
    }
    p.z[l] = (const bf16_t*)L.z;
  }
  for (int l = 0; l < MAXL; ++l) { p.HW[l] = pl.HW[l]; p.chunks[l] = pl.chunks[l]; p.chunk_px[l] = pl.chunk_px[l]; }
  for (int l = 0; l <= MAXL; ++l) { p.first_wg[l] = pl.first_wg[l]; p.first_tile[l] = pl.first_tile[l]; }
  p.n = n; p.B = B; p.C = C; p.C8 = pl.C8; p.cpg = pl.cpg; p.ppp = pl.ppp; p.relu = relu;
  return 0;
}

int sizes_of(const char* who, const tdn_pyr_gn_level* levels, int n, int32_t* hw) {
  TDN_CHECK(levels, "%s: NULL levels", who);
  if (check_levels(who, n, MAXL) != 0) return -1;
  for (int l = 0; l < n; ++l) { hw[2 * l] = levels[l].H; hw[2 * l + 1] = levels[l].W; }
  return 0;
}

// [1] (mode 0; stats is not read) or [1'] (mode 1)
void launch_partial(int mode, int dtype, const PgnArgs& p, int wgs, const float* stats, float* part, void* stream) {
  using Kernel = void (*)(const PgnArgs, const float*, float*);
  static const Kernel kernels[2][2] = {{pgn_partial_kernel<0, false>, pgn_partial_kernel<0, true>},
                                       {pgn_partial_kernel<1, false>, pgn_partial_kernel<1, true>}};
  const Kernel kernel = kernels[mode][dtype == TDN_F16 ? 1 : 0];
  TDN_LAUNCH(kernel, dim3(wgs), dim3(kThreads), 0, stream, p, stats, part);
}

}  // namespace

extern "C" int64_t tdn_pyr_gn_workspace_bytes(int kind, int B, const int32_t* hw, int num_levels, int C, int G) {
  if (check_shape("tdn_pyr_gn_workspace_bytes", kind, B, hw, num_levels, C, G) != 0) return -1;
  PgnPlan pl;
  make_plan(B, hw, num_levels, C, G, pl);
  return ws_layout(kind, pl, num_levels, B, C, nullptr).bytes;
}

extern "C" int tdn_pyr_gn_plan(int kind, int B, const int32_t* hw, int num_levels, int C, int G, int32_t* out32) {
  const char* who = "tdn_pyr_gn_plan";
  int32_t* const out = out32;
  if (check_shape(who, kind, B, hw, num_levels, C, G) != 0) return -1;
  TDN_CHECK(out32, "%s: NULL out", who);
  PgnPlan pl;
  make_plan(B, hw, num_levels, C, G, pl);
  const int64_t ws = ws_layout(kind, pl, num_levels, B, C, nullptr).bytes;
  // out[0..7] chunks per image of each level, out[8..15] pixels per chunk, out[16..18] workgroups of the three launches,
  // out[19] launches, out[20] 16-byte lanes per apply workgroup, out[21] channels per statistics block,
  // out[22], out[23] workspace bytes (low 31 bits, >> 31)
  for (int l = 0; l < MAXL; ++l) { out[l] = pl.chunks[l]; out[MAXL + l] = pl.chunk_px[l]; }
  const int mid = pl.wgs > 0 ? (C / pl.CB) * num_levels * B : 0;
  out[16] = pl.wgs;
  out[17] = mid;
  out[18] = kind == 1 && pl.tiles == 0 ? 1 : pl.tiles;
  out[19] = pl.wgs > 0 ? 3 : (kind == 1 ? 1 : 0);
  out[20] = TILE;
  out[21] = pl.CB;
  put_size(out + 22, ws);
  for (int i = 24; i < 32; ++i) out[i] = 0;
  return 0;
}

extern "C" int tdn_pyr_gn_fwd(const tdn_pyr_gn_level* levels, int num_levels, int B, const float* gamma,
                              const float* beta, int C, int G, float eps, int relu, float* stats, void* workspace,
                              int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_pyr_gn_fwd";
  TDN_CHECK_DTYPE(dtype);
  int32_t hw[2 * MAXL];
  if (sizes_of(who, levels, num_levels, hw) != 0) return -1;
  if (check_shape(who, 0, B, hw, num_levels, C, G) != 0) return -1;
  TDN_CHECK(relu == 0 || relu == 1, "%s: relu=%d is neither 0 nor 1", who, relu);
  PgnPlan pl;
  make_plan(B, hw, num_levels, C, G, pl);
  if (pl.wgs == 0) return 0;
  TDN_CHECK(gamma && beta && stats, "%s: NULL pointer", who);
  const PgnWs ws = ws_layout(0, pl, num_levels, B, C, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, ws.bytes) != 0) return -1;
  PgnArgs p;
  if (fill_args(who, 0, levels, num_levels, B, C, relu, pl, p) != 0) return -1;
  launch_partial(0, dtype, p, pl.wgs, nullptr, ws.part, stream);
  TDN_LAUNCH(pgn_stats_kernel, dim3(C / pl.CB, num_levels * B), dim3(kThreads), 0, stream, p, pl.CB,
             dtype == TDN_F16 ? 1 : 0, (const float*)ws.part, gamma, beta, eps, stats, ws.coef);
  TDN_LAUNCH_T(pgn_apply_kernel, dtype, dim3(pl.tiles), dim3(kThreads), stream, p, (const float*)ws.coef);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_pyr_gn_bwd(const tdn_pyr_gn_level* levels, int num_levels, int B, const float* stats,
                              const float* gamma, int C, int G, int relu, float* dgamma, float* dbeta, float acc,
                              void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_pyr_gn_bwd";
  TDN_CHECK_DTYPE(dtype);
  int32_t hw[2 * MAXL];
  if (sizes_of(who, levels, num_levels, hw) != 0) return -1;
  if (check_shape(who, 1, B, hw, num_levels, C, G) != 0) return -1;
  TDN_CHECK(relu == 0 || relu == 1, "%s: relu=%d is neither 0 nor 1", who, relu);
  TDN_CHECK(gamma && dgamma && dbeta, "%s: NULL pointer", who);
  PgnPlan pl;
  make_plan(B, hw, num_levels, C, G, pl);
  TDN_CHECK(pl.wgs == 0 || (stats && aligned(stats, 16)), "%s: stats must be a 16-byte aligned pointer", who);
  const PgnWs ws = ws_layout(1, pl, num_levels, B, C, workspace);
  if (pl.wgs > 0 && tdn_check_ws(who, workspace, workspace_bytes, ws.bytes) != 0) return -1;
  PgnArgs p;
  if (fill_args(who, 1, levels, num_levels, B, C, relu, pl, p) != 0) return -1;
  if (pl.wgs > 0) {
    launch_partial(1, dtype, p, pl.wgs, stats, ws.part, stream);
    TDN_LAUNCH(pgn_bwd_coef_kernel, dim3(C / pl.CB, num_levels * B), dim3(kThreads), 0, stream, p, pl.CB,
               (const float*)ws.part, gamma, stats, ws.coef, ws.sums);
  }
  TDN_LAUNCH_T(pgn_bwd_apply_kernel, dtype, dim3(pl.tiles > 0 ? pl.tiles : 1), dim3(kThreads), stream, p, pl.tiles,
               (const float*)ws.coef, stats, (const float*)ws.sums, dgamma, dbeta, acc);
  TDN_LAUNCH_CHECK();
  return 0;
}
