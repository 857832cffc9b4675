// The box delta encode and decode of DESIGN.md §4b, shared by tdn_bbox2delta / tdn_delta2bbox and the RPN proposals
// (proposal.hip), the training-target kernels (target.hip) and the test-time detections (detect.hip): spec order, one
// rounding per operation.  Every one of these translation units is compiled with -ffp-contract=off.
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

// ---- decode (spec order, one rounding per operation) ----------------------------------------------------------------
// clip_w < 0: no clipping
__device__ __forceinline__ f32x4_t decode_box(const f32x4_t r, const f32x4_t delta, const f32x4_t means,
                                              const f32x4_t stds, float max_ratio, int clip_h, int clip_w) {
  f32x4_t d;
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = __fadd_rn(__fmul_rn(delta[e], stds[e]), means[e]);
  const float dw = fminf(fmaxf(d[2], -max_ratio), max_ratio), dh = fminf(fmaxf(d[3], -max_ratio), max_ratio);
  const float px = __fmul_rn(__fadd_rn(r[0], r[2]), 0.5f), py = __fmul_rn(__fadd_rn(r[1], r[3]), 0.5f);
  const float pw = __fadd_rn(__fsub_rn(r[2], r[0]), 1.0f), ph = __fadd_rn(__fsub_rn(r[3], r[1]), 1.0f);
  const float gw = __fmul_rn(pw, expf(dw)), gh = __fmul_rn(ph, expf(dh));
  const float gx = __fadd_rn(px, __fmul_rn(pw, d[0])), gy = __fadd_rn(py, __fmul_rn(ph, d[1]));
  const float hw = __fmul_rn(gw, 0.5f), hh = __fmul_rn(gh, 0.5f);
  f32x4_t o;
  o[0] = __fadd_rn(__fsub_rn(gx, hw), 0.5f);
  o[1] = __fadd_rn(__fsub_rn(gy, hh), 0.5f);
  o[2] = __fsub_rn(__fadd_rn(gx, hw), 0.5f);
  o[3] = __fsub_rn(__fadd_rn(gy, hh), 0.5f);
  if (clip_w >= 0) {
    const float xm = (float)(clip_w - 1), ym = (float)(clip_h - 1);
    o[0] = fminf(fmaxf(o[0], 0.f), xm);
    o[1] = fminf(fmaxf(o[1], 0.f), ym);
    o[2] = fminf(fmaxf(o[2], 0.f), xm);
    o[3] = fminf(fmaxf(o[3], 0.f), ym);
  }
  return o;
}
