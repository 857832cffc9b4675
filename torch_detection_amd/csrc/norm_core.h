// The statistics of the normalisation kernels, stated once: gn.hip (GroupNorm and training-mode BatchNorm of one map)
// and pyramid_gn.hip (GroupNorm over a pyramid) run the same three passes and take the chunk cut, the totals of pass [2]
// and the group arithmetic from here.  The order of every floating-point operation and LDS reduction below is part of
// the contract: a level gives the same bits through either file (DESIGN.md "Numerics of the statistics", §4o).
#pragma once
#include "common.h"

constexpr int kThreads = 256;

// ---- the chunk cut of one map: a function of (B, HW, C / 8) only -------------------------------------------------------
// A block's 256 threads are C8 channel lanes (8 channels, 16 bytes) x ppp pixel lanes.  About 1024 blocks in flight over
// the batch, at least four passes of the pixel lanes per block; `chunks` is recomputed so that the last one is not empty.
struct Cut { int ppp, chunks, chunk_px; };
static inline int pixel_lanes(int C8) { return kThreads / C8; }
static inline Cut cut_of(int B, int HW, int C8) {
  Cut c;
  c.ppp = pixel_lanes(C8);
  int chunks = ceil_div(1024, B);
  const int max_chunks = ceil_div(HW, c.ppp * 4);
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks < 1) chunks = 1;
  c.chunk_px = ceil_div(HW, chunks);
  c.chunks = ceil_div(HW, c.chunk_px);
  return c;
}

// ---- [2] / [2']: totals of channel c over `count` rows of `part` -------------------------------------------------------
// rows: the first of `count` consecutive [2][C] rows.  A block is CB channels x KL row lanes, CB * KL = kThreads; CB
// divides C (both powers of two, C >= 64, CB = max(32, cpg) <= 256), so every thread has a channel.  Thread (cl, kl) takes
// rows kl, kl + KL, ...; the lanes are combined through LDS in lane order; threads with kl == 0 get both planes' totals.
// No barrier follows the last read of `red`: a caller that reuses it orders that.
__device__ __forceinline__ void row_totals(const float* __restrict__ rows, int count, int C, int c, int cl, int kl, int CB,
                                           int KL, double* red /*[2][kThreads]*/, double& s, double& ss) {
  double a = 0.0, b = 0.0;
  for (int k = kl; k < count; k += KL) {
    const float* q = rows + (int64_t)k * 2 * C + c;
    a += (double)q[0];
    b += (double)q[C];
  }
  red[kl * CB + cl] = a;
  red[kThreads + kl * CB + cl] = b;
  __syncthreads();
  s = 0.0; ss = 0.0;
  if (kl == 0) {
    for (int j = 0; j < KL; ++j) { s += red[j * CB + cl]; ss += red[kThreads + j * CB + cl]; }
  }
}

// the pivot of a channel as the partial kernel read it; zc: the channel's element at pixel 0
__device__ __forceinline__ double pivot_of(const bf16_t* zc, int f16) {
  return (double)(f16 ? elem_to_f32<true>(*zc) : elem_to_f32<false>(*zc));
}

// 1 / sqrt(var + eps) of a biased variance, which is first clamped at 0 in place
__device__ __forceinline__ float rstd_of(double& var, float eps) {
  if (var < 0.0) var = 0.0;
  return (float)(1.0 / sqrt(var + (double)eps));
}

// Mean and rstd of the group of cpg channels that starts at block-local channel g0, from tot[3][kThreads] = the
// channels' (s_c, q_c, K_c): s_c = sum (z - K_c), q_c = sum (z - K_c)^2 over the HW pixels of channel c.
//   mu = sum_c (s_c + HW K_c) / cnt,   cnt var = sum_c (q_c + 2 (K_c - mu) s_c + HW (K_c - mu)^2)
// (the second moment about the group mean, cross terms between the channels' pivots included), in channel order, in
// double; biased variance, like nn.GroupNorm.
struct Moments { double mu; float rstd; };
__device__ __forceinline__ Moments group_moments(const double* tot, int g0, int cpg, int HW, float eps) {
  const double hw = (double)HW, cnt = hw * cpg;
  double gs = 0.0;
  for (int j = 0; j < cpg; ++j) gs += tot[g0 + j] + hw * tot[2 * kThreads + g0 + j];
  const double mu = gs / cnt;
  double m2 = 0.0;
  for (int j = 0; j < cpg; ++j) {
    const double dk = tot[2 * kThreads + g0 + j] - mu;
    m2 += tot[kThreads + g0 + j] + 2.0 * dk * tot[g0 + j] + hw * dk * dk;
  }
  double var = m2 / cnt;
  return Moments{mu, rstd_of(var, eps)};
}

// The affine of y = (z - K) * a + b':  a = rstd gamma,  b' = beta - (mu - K) a  formed in double.  dmu = mu - K.
__device__ __forceinline__ void fwd_coef(float rstd, float gamma, float beta, double dmu, float& a, float& b) {
  a = rstd * gamma;
  b = (float)((double)beta - dmu * (double)a);
}

// [2']: the group means m1 = sum_c gamma s1 / cnt, m2 = sum_c gamma s2 / cnt from t1[] = gamma s1, t2[] = gamma s2 of the
// cpg channels that start at block-local channel l0, in channel order
__device__ __forceinline__ void group_means(const float* t1, const float* t2, int l0, int cpg, float cnt, float& m1,
                                            float& m2) {
  m1 = 0.f; m2 = 0.f;
  for (int j = 0; j < cpg; ++j) { m1 += t1[l0 + j]; m2 += t2[l0 + j]; }
  m1 /= cnt; m2 /= cnt;
}

