// GroupNorm forward / backward on NHWC 16-bit activations (gfx950).
//
// Replaces nn.GroupNorm(get_group_gn(planes), planes) as built by models/utils/layers.py:50-54,138-154 (32 groups)
// and applied after the convs of models/backbone/resnet.py (use_gn=True: :42-59, :97-119, :254-257) and of ConvModule
// (layers.py:122-135, necks with normalize=GN), together with the residual add and ReLU that follow it.
// Unlike eval-mode BatchNorm the statistics depend on the sample, so GN cannot be folded into the conv epilogue:
//   forward   z = conv(x) (raw, 16-bit)  ->  [1] per-channel partial (sum, sum of squares) of z - K over pixel chunks,
//                K = the channel's pivot: its value at pixel 0 of the sample (GN) / of sample 0 (BN)
//             -> [2] per (sample, group) mean / rstd, expanded to per-(sample, channel) affine (a, b, K)
//             -> [3] y = relu?((z - K)*a + b (+ addend))      (relu: 0 none, 1 ReLU, 2 ReLU6)
//   Numerics of the statistics (GroupNorm): the fp32 sums are taken about the pivot, so they carry the
//   spread of the data and not its offset: sum z^2 / cnt - mu^2 would cancel |mean|^2 / var leading digits, which a
//   16-bit tensor can make 2^20.  The pivots are put back in double in [2].  The output is formed about the same pivot
//   for the same reason: z*a - mu*a would round at the size of |mean| * a.
//   backward  g = dL/dy (ReLU-masked) -> [1'] per-channel partial (sum g, sum g*xhat) -> [2'] dgamma, dbeta and the
//             per-(sample, channel) coefficients of dz = g*A + z*B + C  ->  [3'] dz, which then feeds the ordinary
//             conv dgrad / wgrad kernels.
// All three passes are HBM-bound streams, 16 bytes (8 channels) per lane; reductions are fixed-order (deterministic).
#include "norm_core.h"

namespace {

struct GnGeom {
  int N, HW, C, G, cpg;      // cpg = C / G channels per group
  int C8;                    // C / 8 lanes per pixel
  int ppp;                   // pixels per pass of one 256-thread block
  int chunks, chunk_px;      // pixel chunks per sample, pixels per chunk: norm_core.h's cut_of
};

// [1] / [1']: partial per-channel sums over one pixel chunk of one sample.
//   MODE 0: (sum d, sum d^2), d = z - K, K = z[n * pivot_stride + c] (pixel 0 of the sample, or of sample 0)
//   MODE 1: (sum g, sum g * xhat), xhat = (z - mu) * rstd from `stats`
// part layout: [n][chunk][2][C]
template <int MODE, bool F16>
__global__ __launch_bounds__(kThreads) void gn_partial_kernel(const bf16_t* __restrict__ z,
                                                               const bf16_t* __restrict__ g,
                                                               const float* __restrict__ stats, GnGeom ge,
                                                               int64_t pivot_stride, float* __restrict__ part) {
  __shared__ float red[kThreads][17];
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int tid = threadIdx.x;
  const int cl = tid % ge.C8, pl = tid / ge.C8;   // channel lane (8 channels), pixel lane
  const int p0 = chunk * ge.chunk_px;
  const int p1 = min(ge.HW, p0 + ge.chunk_px);
  float a0[8], a1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
  float mu[8], rs[8];
  if (MODE == 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      mu[e] = stats[((int64_t)n * ge.C + cl * 8 + e) * 2];
      rs[e] = stats[((int64_t)n * ge.C + cl * 8 + e) * 2 + 1];
    }
  }
  const int64_t base = (int64_t)n * ge.HW * ge.C + cl * 8;
  float piv[8];
  if (MODE == 0) {
    const bf16x8_t kv = *(const bf16x8_t*)(z + (int64_t)n * pivot_stride + cl * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) piv[e] = elem_to_f32<F16>(kv[e]);
  }
  for (int p = p0 + pl; p < p1; p += ge.ppp) {
    const bf16x8_t zv = *(const bf16x8_t*)(z + base + (int64_t)p * ge.C);
    if (MODE == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = elem_to_f32<F16>(zv[e]) - piv[e];
        a0[e] += d;
        a1[e] += d * d;
      }
    } else {
      const bf16x8_t gv = *(const bf16x8_t*)(g + base + (int64_t)p * ge.C);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gg = elem_to_f32<F16>(gv[e]);
        const float xh = (elem_to_f32<F16>(zv[e]) - mu[e]) * rs[e];   // z*rstd - mu*rstd would round at |z| * rstd
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
    for (int j = 1; j < ge.ppp; ++j) {
#pragma unroll
      for (int e = 0; e < 16; ++e) red[tid][e] += red[j * ge.C8 + cl][e];
    }
    float* o = part + (((int64_t)n * ge.chunks + chunk) * 2) * ge.C + cl * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { o[e] = red[tid][e]; o[ge.C + e] = red[tid][8 + e]; }
  }
}

// [2]: block (sample n, channel block of CB = max(32, cpg) channels — whole groups); chunk sums -> group mean / rstd
// (norm_core.h's group_moments), then per-channel stats[n][c] = (mu, rstd) and the three planes coef[3][n][c] = a, b, K of
// y = (z - K)*a + b (planes: a lane's 8 channels are 32 contiguous bytes of each, fewer cache lines than [n][c][3]).
__global__ __launch_bounds__(kThreads) void gn_stats_kernel(const float* __restrict__ part, GnGeom ge, int CB,
                                                            const bf16_t* __restrict__ z, int f16,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps,
                                                            float* __restrict__ stats, float* __restrict__ coef) {
  __shared__ double red[2 * kThreads];
  __shared__ double tot[3 * kThreads];
  const int n = blockIdx.y;
  const int KL = kThreads / CB;
  const int cl = threadIdx.x % CB, kl = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cl;               // < C: CB divides C
  const bf16_t* zc = z + (int64_t)n * ge.HW * ge.C + c;
  const double K = kl == 0 ? pivot_of(zc, f16) : 0.0;     // asked for ahead of the chunk sums: its latency hides
  double s, ss;
  row_totals(part + (int64_t)n * ge.chunks * 2 * ge.C, ge.chunks, ge.C, c, cl, kl, CB, KL, red, s, ss);
  if (kl == 0) { tot[cl] = s; tot[kThreads + cl] = ss; tot[2 * kThreads + cl] = K; }
  __syncthreads();
  if (kl == 0) {
    const Moments m = group_moments(tot, (cl / ge.cpg) * ge.cpg, ge.cpg, ge.HW, eps);
    stats[((int64_t)n * ge.C + c) * 2] = (float)m.mu;
    stats[((int64_t)n * ge.C + c) * 2 + 1] = m.rstd;
    float a, b;
    fwd_coef(m.rstd, gamma[c], beta[c], m.mu - K, a, b);
    float* o = coef + (int64_t)n * ge.C + c;
    const int64_t plane = (int64_t)ge.N * ge.C;
    o[0] = a;
    o[plane] = b;
    o[2 * plane] = (float)K;
  }
}

// [3]: y = relu?((z - K)*a + b (+ addend)), coef[3][n][c] = a, b, K;  up_w > 0: the addend is the coarser FPN level
// (H/2 x W/2), read with nearest-neighbour 2x upsampling (fpn.py:98-100), W = 2*up_w
template <bool F16>
__global__ void gn_apply_kernel(const bf16_t* __restrict__ z, const float* __restrict__ coef,
                                const bf16_t* __restrict__ addend, int relu, int up_w, GnGeom ge,
                                bf16_t* __restrict__ y) {
  const int64_t per_n = (int64_t)ge.HW * ge.C8, total = per_n * ge.N;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / per_n);
    const int cl = (int)(i % ge.C8);
    const bf16x8_t zv = *(const bf16x8_t*)(z + i * 8);
    const float* cf = coef + (int64_t)n * ge.C + cl * 8;
    const int64_t plane = (int64_t)ge.N * ge.C;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4_t ca = *(const f32x4_t*)(cf + 4 * h), cb = *(const f32x4_t*)(cf + plane + 4 * h);
      const f32x4_t ck = *(const f32x4_t*)(cf + 2 * plane + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * h + e] = (elem_to_f32<F16>(zv[4 * h + e]) - ck[e]) * ca[e] + cb[e];
    }
    if (addend) {
      int64_t ai = i;
      if (up_w > 0) {
        const int W = 2 * up_w;
        const int64_t pix = (i - (int64_t)n * per_n) / ge.C8;
        const int h = (int)(pix / W), w = (int)(pix - (int64_t)h * W);
        ai = (((int64_t)n * (ge.HW / 4)) + (int64_t)(h >> 1) * up_w + (w >> 1)) * ge.C8 + cl;
      }
      const bf16x8_t av = *(const bf16x8_t*)(addend + ai * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += elem_to_f32<F16>(av[e]);
    }
    bf16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = relu ? fmaxf(v[e], 0.f) : v[e];
      if (relu == 2) t = relu6_top<F16>(t);       // nn.ReLU6
      o[e] = f32_to_elem<F16>(t);
    }
    *(bf16x8_t*)(y + i * 8) = o;
  }
}

// [2']: block = channel block of CB = max(32, cpg) channels (whole groups), all samples in turn: chunk sums ->
// (s1, s2), group means m1 = sum_c gamma*s1 / cnt, m2 = sum_c gamma*s2 / cnt, coefficients of dz = g*A + z*B + Cc;
// across samples: dgamma = sum_n s2, dbeta = sum_n s1.
__global__ __launch_bounds__(kThreads) void gn_bwd_coef_kernel(const float* __restrict__ part, GnGeom ge, int CB,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ stats,
                                                               float* __restrict__ coef3, float* dgamma, float* dbeta,
                                                               float acc) {
  __shared__ double red[2 * kThreads];
  __shared__ float t1[kThreads], t2[kThreads];
  const int KL = kThreads / CB;
  const int cl = threadIdx.x % CB, kl = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cl;               // < C: CB divides C
  const float gm = gamma[c];
  float dg = 0.f, db = 0.f;
  const float cnt = (float)ge.HW * (float)ge.cpg;
  for (int n = 0; n < ge.N; ++n) {
    // `red` is written again here: its last read, inside row_totals of the previous sample, is followed by the two
    // barriers below, and t1 / t2 are written only after the barrier inside row_totals, which follows their last read
    double d1, d2;
    row_totals(part + (int64_t)n * ge.chunks * 2 * ge.C, ge.chunks, ge.C, c, cl, kl, CB, KL, red, d1, d2);
    const float s1 = (float)d1, s2 = (float)d2;
    if (kl == 0) {
      dg += s2;
      db += s1;
      t1[cl] = gm * s1;
      t2[cl] = gm * s2;
    }
    __syncthreads();
    if (kl == 0) {
      float m1, m2;
      group_means(t1, t2, (cl / ge.cpg) * ge.cpg, ge.cpg, cnt, m1, m2);
      const float mu = stats[((int64_t)n * ge.C + c) * 2], r = stats[((int64_t)n * ge.C + c) * 2 + 1];
      float* o = coef3 + ((int64_t)n * ge.C + c) * 3;
      o[0] = r * gm;                       // A
      o[1] = -r * r * m2;                  // B
      o[2] = -r * m1 + mu * r * r * m2;    // C
    }
    __syncthreads();
  }
  if (kl == 0) {
    dgamma[c] = (acc != 0.f) ? acc * dgamma[c] + dg : dg;
    dbeta[c] = (acc != 0.f) ? acc * dbeta[c] + db : db;
  }
}

// [3']: dz = g*A + z*B + C
template <bool F16>
__global__ void gn_bwd_apply_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ z,
                                    const float* __restrict__ coef3, GnGeom ge, bf16_t* __restrict__ dz) {
  const int64_t per_n = (int64_t)ge.HW * ge.C8, total = per_n * ge.N;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / per_n);
    const int cl = (int)(i % ge.C8);
    const bf16x8_t gv = *(const bf16x8_t*)(g + i * 8);
    const bf16x8_t zv = *(const bf16x8_t*)(z + i * 8);
    const float* cf = coef3 + ((int64_t)n * ge.C + cl * 8) * 3;
    bf16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = f32_to_elem<F16>(elem_to_f32<F16>(gv[e]) * cf[3 * e] + elem_to_f32<F16>(zv[e]) * cf[3 * e + 1] +
                              cf[3 * e + 2]);
    *(bf16x8_t*)(dz + i * 8) = o;
  }
}

// ---- training-mode BatchNorm2d (batch statistics): the same three passes with the statistics taken per channel over
// the whole batch (N, H, W) instead of per (sample, group).  Only the two small middle kernels differ; stats / coef
// are still written per (sample, channel) — identical for every sample — so the element-wise passes are shared. ----
// A block is CB = 32 channels (32 divides C); its totals run over ALL samples and chunks of a channel: [n][chunk] is
// one flat index of the rows of the partials.
// The pivot K_c is common to all samples (sample 0's pixel 0): mu = K_c + s / cnt, var = q / cnt - (s / cnt)^2 with
// s, q the sums of z - K_c and its square over the batch, both of the size of the spread.
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const float* __restrict__ part, GnGeom ge,
                                                            const bf16_t* __restrict__ z, int f16,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, float momentum,
                                                            float* running_mean, float* running_var,
                                                            float* __restrict__ stats, float* __restrict__ coef) {
  __shared__ double red[2 * kThreads];
  constexpr int CB = 32, KL = kThreads / CB;
  const int cl = threadIdx.x % CB, kl = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cl;
  const double K = kl == 0 ? pivot_of(z + c, f16) : 0.0;   // ahead of the sums: its latency hides
  double s, ss;
  row_totals(part, ge.N * ge.chunks, ge.C, c, cl, kl, CB, KL, red, s, ss);
  if (kl != 0) return;
  const double cnt = (double)ge.N * ge.HW;
  const double dm = s / cnt;
  const double mu = K + dm;
  double var = ss / cnt - dm * dm;             // biased variance normalises (nn.BatchNorm2d, training)
  const float rstd = rstd_of(var, eps);
  const float muf = (float)mu;
  float a, b;
  fwd_coef(rstd, gamma[c], beta[c], dm, a, b);
  for (int n = 0; n < ge.N; ++n) {
    stats[((int64_t)n * ge.C + c) * 2] = muf;
    stats[((int64_t)n * ge.C + c) * 2 + 1] = rstd;
    float* o = coef + (int64_t)n * ge.C + c;
    const int64_t plane = (int64_t)ge.N * ge.C;
    o[0] = a;
    o[plane] = b;
    o[2 * plane] = (float)K;
  }
  if (running_mean && running_var) {           // running statistics: unbiased variance, momentum update
    const double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * muf;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
  }
}

// bn_bwd_coef_kernel's own copy of row_totals(part, N * chunks, ...), dead `live` predicate included: with the shared
// one this kernel is allocated more registers (profiles/norm_core_refactor_checks.md §2), so it keeps its old text.
__device__ __forceinline__ void batch_totals(const float* __restrict__ part, const GnGeom& ge, int c, int cl, int kl,
                                             int CB, int KL, bool live, double* red, double& s, double& ss) {
  double a = 0.0, b = 0.0;
  if (live) {
    for (int k = kl; k < ge.N * ge.chunks; k += KL) {
      const float* q = part + ((int64_t)k * 2) * ge.C + c;
      a += (double)q[0];
      b += (double)q[ge.C];
    }
  }
  red[kl * CB + cl] = a;
  red[kThreads + kl * CB + cl] = b;
  __syncthreads();
  s = 0.0; ss = 0.0;
  if (kl == 0) {
    for (int j = 0; j < KL; ++j) { s += red[j * CB + cl]; ss += red[kThreads + j * CB + cl]; }
  }
}

__global__ __launch_bounds__(kThreads) void bn_bwd_coef_kernel(const float* __restrict__ part, GnGeom ge,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ stats,
                                                               float* __restrict__ coef3, float* dgamma, float* dbeta,
                                                               float acc) {
  __shared__ double red[2 * kThreads];
  constexpr int CB = 32, KL = kThreads / CB;
  const int cl = threadIdx.x % CB, kl = threadIdx.x / CB;
  const int c = blockIdx.x * CB + cl;
  double d1, d2;
  batch_totals(part, ge, c, cl, kl, CB, KL, c < ge.C, red, d1, d2);
  if (kl != 0 || c >= ge.C) return;
  const float s1 = (float)d1, s2 = (float)d2;
  const float gm = gamma[c];
  const float cnt = (float)ge.N * (float)ge.HW;
  const float m1 = gm * s1 / cnt, m2 = gm * s2 / cnt;
  const float mu = stats[(int64_t)c * 2], r = stats[(int64_t)c * 2 + 1];
  for (int n = 0; n < ge.N; ++n) {
    float* o = coef3 + ((int64_t)n * ge.C + c) * 3;
    o[0] = r * gm;
    o[1] = -r * r * m2;
    o[2] = -r * m1 + mu * r * r * m2;
  }
  dgamma[c] = (acc != 0.f) ? acc * dgamma[c] + s2 : s2;
  dbeta[c] = (acc != 0.f) ? acc * dbeta[c] + s1 : s1;
}

int make_geom(GnGeom& ge, int N, int H, int W, int C, int G) {
  TDN_CHECK(N > 0 && H > 0 && W > 0, "GroupNorm: bad shape N=%d H=%d W=%d", N, H, W);
  TDN_CHECK(C >= 64 && C <= 2048 && (C & (C - 1)) == 0, "GroupNorm: C=%d must be a power of two in 64..2048", C);
  TDN_CHECK(G > 0 && C % G == 0, "GroupNorm: %d groups do not divide %d channels", G, C);
  ge.N = N; ge.HW = H * W; ge.C = C; ge.G = G; ge.cpg = C / G;
  TDN_CHECK((ge.cpg & (ge.cpg - 1)) == 0 && ge.cpg <= 256, "GroupNorm: %d channels per group not supported", ge.cpg);
  ge.C8 = C / 8;
  const Cut cut = cut_of(N, ge.HW, ge.C8);
  ge.ppp = cut.ppp; ge.chunks = cut.chunks; ge.chunk_px = cut.chunk_px;
  return 0;
}

// workspace: part [N][chunks][2][C] floats | coef: 3 N C floats (forward: planes [3][N][C], backward: [N][C][3])
struct GnWs { float* part; float* coef; int64_t bytes; };
GnWs ws_layout(const GnGeom& ge, void* base) {
  const int64_t part_floats = (int64_t)ge.N * ge.chunks * 2 * ge.C, coef_floats = (int64_t)ge.N * ge.C * 3;
  return GnWs{(float*)base, base ? (float*)base + part_floats : nullptr, (part_floats + coef_floats) * 4};
}

// the geometry of a call and its workspace, checked
int prepare(const char* who, int N, int H, int W, int C, int G, void* workspace, int64_t workspace_bytes, GnGeom& ge,
            GnWs& ws) {
  if (make_geom(ge, N, H, W, C, G)) return -1;
  ws = ws_layout(ge, workspace);
  TDN_CHECK(workspace_bytes >= ws.bytes && ((uintptr_t)workspace & 15) == 0, "%s: workspace too small or misaligned",
            who);
  return 0;
}

// the addend of a forward -> up_w: W / 2 if it is the coarser level read with 2x upsampling, else 0; -1: refused
int addend_up_w(const char* who, const void* addend, int addend_mode, int H, int W) {
  TDN_CHECK(!addend || addend_mode == TDN_ADD_SAME || addend_mode == TDN_ADD_UP2X,
            "%s: addend_mode %d (TDN_ADD_SAME or TDN_ADD_UP2X)", who, addend_mode);
  TDN_CHECK(!(addend && addend_mode == TDN_ADD_UP2X) || (H % 2 == 0 && W % 2 == 0),
            "%s: UP2X addend needs even H, W (got %dx%d)", who, H, W);
  return (addend && addend_mode == TDN_ADD_UP2X) ? W / 2 : 0;
}

// [1] (mode 0; g and stats are not read) or [1'] (mode 1; pivot_stride is not read)
void launch_partial(int mode, int dtype, const GnGeom& ge, const void* z, const void* g, const float* stats,
                    int64_t pivot_stride, float* part, hipStream_t st) {
  using Kernel = void (*)(const bf16_t*, const bf16_t*, const float*, GnGeom, int64_t, float*);
  static const Kernel kernels[2][2] = {{gn_partial_kernel<0, false>, gn_partial_kernel<0, true>},
                                       {gn_partial_kernel<1, false>, gn_partial_kernel<1, true>}};
  const Kernel kernel = kernels[mode][dtype == TDN_F16 ? 1 : 0];
  TDN_LAUNCH(kernel, dim3(ge.chunks, ge.N), dim3(kThreads), 0, st, (const bf16_t*)z, (const bf16_t*)g, stats, ge,
             pivot_stride, part);
}

// grid of the grid-stride apply kernels [3] / [3']
dim3 apply_grid(const GnGeom& ge) {
  const int64_t total = (int64_t)ge.N * ge.HW * ge.C8;
  int grid = (int)((total + kThreads - 1) / kThreads);
  if (grid > 8192) grid = 8192;
  return dim3(grid);
}

int stats_block(const GnGeom& ge) { return ge.cpg > 32 ? ge.cpg : 32; }   // channels per block of [2] / [2']: divides C

}  // namespace

extern "C" int64_t tdn_gn_workspace(int N, int H, int W, int C, int G) {
  GnGeom ge;
  if (make_geom(ge, N, H, W, C, G)) return -1;
  return ws_layout(ge, nullptr).bytes + 256;
}

extern "C" int tdn_gn_fwd(const void* z, const float* gamma, const float* beta, int N, int H, int W, int C, int G,
                          float eps, const void* addend, int addend_mode, int relu, void* y, float* stats,
                          void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_gn_fwd";
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(z && gamma && beta && y && stats && workspace, "%s: NULL pointer", who);
  GnGeom ge;
  GnWs ws;
  const int up_w = addend_up_w(who, addend, addend_mode, H, W);
  if (up_w < 0) return -1;
  if (prepare(who, N, H, W, C, G, workspace, workspace_bytes, ge, ws)) return -1;
  hipStream_t st = (hipStream_t)stream;
  launch_partial(0, dtype, ge, z, nullptr, nullptr, (int64_t)ge.HW * ge.C, ws.part, st);
  const int CB = stats_block(ge);
  TDN_LAUNCH(gn_stats_kernel, dim3(C / CB, N), dim3(kThreads), 0, st, (const float*)ws.part, ge, CB, (const bf16_t*)z,
             dtype == TDN_F16 ? 1 : 0, gamma, beta, eps, stats, ws.coef);
  TDN_LAUNCH_T(gn_apply_kernel, dtype, apply_grid(ge), dim3(kThreads), st, (const bf16_t*)z, (const float*)ws.coef,
               (const bf16_t*)addend, relu, up_w, ge, (bf16_t*)y);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_gn_bwd(const void* g, const void* z, const float* stats, const float* gamma, int N, int H, int W,
                          int C, int G, void* dz, float* dgamma, float* dbeta, float acc, void* workspace,
                          int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_gn_bwd";
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(g && z && stats && gamma && dz && dgamma && dbeta && workspace, "%s: NULL pointer", who);
  GnGeom ge;
  GnWs ws;
  if (prepare(who, N, H, W, C, G, workspace, workspace_bytes, ge, ws)) return -1;
  hipStream_t st = (hipStream_t)stream;
  launch_partial(1, dtype, ge, z, g, stats, 0, ws.part, st);
  const int CB = stats_block(ge);
  TDN_LAUNCH(gn_bwd_coef_kernel, dim3(C / CB), dim3(kThreads), 0, st, (const float*)ws.part, ge, CB, gamma, stats,
             ws.coef, dgamma, dbeta, acc);
  TDN_LAUNCH_T(gn_bwd_apply_kernel, dtype, apply_grid(ge), dim3(kThreads), st, (const bf16_t*)g, (const bf16_t*)z,
               (const float*)ws.coef, ge, (bf16_t*)dz);
  TDN_LAUNCH_CHECK();
  return 0;
}

// Training-mode nn.BatchNorm2d (models/utils/layers.py:50-54 with ResNet(bn_eval=False), resnet.py:270-276): batch
// statistics over (N, H, W), running statistics updated in place (momentum; unbiased variance) when given.
// Workspace: tdn_gn_workspace(N, H, W, C, C).
extern "C" int tdn_bn_train_fwd(const void* z, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, float momentum, int N, int H, int W, int C, float eps,
                                const void* addend, int addend_mode, int relu, void* y, float* stats, void* workspace,
                                int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_bn_train_fwd";
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(z && gamma && beta && y && stats && workspace, "%s: NULL pointer", who);
  TDN_CHECK((running_mean == nullptr) == (running_var == nullptr), "%s: give both running stats or none", who);
  GnGeom ge;
  GnWs ws;
  const int up_w = addend_up_w(who, addend, addend_mode, H, W);
  if (up_w < 0) return -1;
  if (prepare(who, N, H, W, C, C, workspace, workspace_bytes, ge, ws)) return -1;
  hipStream_t st = (hipStream_t)stream;
  launch_partial(0, dtype, ge, z, nullptr, nullptr, 0, ws.part, st);
  TDN_LAUNCH(bn_stats_kernel, dim3(C / 32), dim3(kThreads), 0, st, (const float*)ws.part, ge, (const bf16_t*)z,
             dtype == TDN_F16 ? 1 : 0, gamma, beta, eps, momentum, running_mean, running_var, stats, ws.coef);
  TDN_LAUNCH_T(gn_apply_kernel, dtype, apply_grid(ge), dim3(kThreads), st, (const bf16_t*)z, (const float*)ws.coef,
               (const bf16_t*)addend, relu, up_w, ge, (bf16_t*)y);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_bn_train_bwd(const void* g, const void* z, const float* stats, const float* gamma, int N, int H,
                                int W, int C, void* dz, float* dgamma, float* dbeta, float acc, void* workspace,
                                int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_bn_train_bwd";
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(g && z && stats && gamma && dz && dgamma && dbeta && workspace, "%s: NULL pointer", who);
  GnGeom ge;
  GnWs ws;
  if (prepare(who, N, H, W, C, C, workspace, workspace_bytes, ge, ws)) return -1;
  hipStream_t st = (hipStream_t)stream;
  launch_partial(1, dtype, ge, z, g, stats, 0, ws.part, st);
  TDN_LAUNCH(bn_bwd_coef_kernel, dim3(C / 32), dim3(kThreads), 0, st, (const float*)ws.part, ge, gamma, stats, ws.coef,
             dgamma, dbeta, acc);
  TDN_LAUNCH_T(gn_bwd_apply_kernel, dtype, apply_grid(ge), dim3(kThreads), st, (const bf16_t*)g, (const bf16_t*)z,
               (const float*)ws.coef, ge, (bf16_t*)dz);
  TDN_LAUNCH_CHECK();
  return 0;
}
