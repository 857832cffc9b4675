// The box delta encode of DESIGN.md §4b, shared by tdn_bbox2delta (proposal.hip) and the training-target kernels
// (target.hip): spec order, one rounding per operation.  Both translation units are compiled with -ffp-contract=off.
#pragma once
#include "common.h"
#include <math.h>

__device__ __forceinline__ f32x4_t encode_box(const f32x4_t p, const f32x4_t g, const f32x4_t means,
                                              const f32x4_t stds) {
  const float px = __fmul_rn(__fadd_rn(p[0], p[2]), 0.5f), py = __fmul_rn(__fadd_rn(p[1], p[3]), 0.5f);
  const float pw = __fadd_rn(__fsub_rn(p[2], p[0]), 1.0f), ph = __fadd_rn(__fsub_rn(p[3], p[1]), 1.0f);
  const float gx = __fmul_rn(__fadd_rn(g[0], g[2]), 0.5f), gy = __fmul_rn(__fadd_rn(g[1], g[3]), 0.5f);
  const float gw = __fadd_rn(__fsub_rn(g[2], g[0]), 1.0f), gh = __fadd_rn(__fsub_rn(g[3], g[1]), 1.0f);
  f32x4_t d;
  d[0] = __fdiv_rn(__fsub_rn(gx, px), pw);
  d[1] = __fdiv_rn(__fsub_rn(gy, py), ph);
  d[2] = logf(__fdiv_rn(gw, pw));
  d[3] = logf(__fdiv_rn(gh, ph));
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = __fdiv_rn(__fsub_rn(d[e], means[e]), stds[e]);
  return d;
}
