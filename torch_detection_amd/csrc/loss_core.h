// The elementwise spec of the sigmoid classification losses, shared by loss.hip and fcos.hip: fp32 with
// explicit __f*_rn arithmetic in the order written (both files are compiled with -ffp-contract=off); with it the storage
// types of the head outputs and the lane reduction of the fp64 sums.
#pragma once
#include "common.h"

__device__ __forceinline__ float e_neg_abs(float z) { return expf(-fabsf(z)); }
__device__ __forceinline__ float softplus(float z) { return __fadd_rn(fmaxf(z, 0.f), log1pf(e_neg_abs(z))); }
__device__ __forceinline__ float sigmoid(float z) {
  const float e = e_neg_abs(z);
  const float d = __fadd_rn(1.f, e);
  return z >= 0.f ? __fdiv_rn(1.f, d) : __fdiv_rn(e, d);
}

struct ClsParams {
  int focal;
  float gamma, alpha, one_minus_alpha;
};

// GRAD: d loss / d logit, else the loss; t: the element's class is the anchor's label
template <bool GRAD>
__device__ __forceinline__ float cls_elem(float x, bool t, const ClsParams& P) {
  if (!P.focal) {
    if (GRAD) return t ? -sigmoid(-x) : sigmoid(x);
    return t ? softplus(-x) : softplus(x);
  }
  if (t) {
    const float mod = __fmul_rn(P.alpha, expf(-__fmul_rn(P.gamma, softplus(x))));
    if (!GRAD) return __fmul_rn(mod, softplus(-x));
    const float inner = __fadd_rn(__fmul_rn(__fmul_rn(P.gamma, sigmoid(x)), softplus(-x)), sigmoid(-x));
    return -__fmul_rn(mod, inner);
  }
  const float mod = __fmul_rn(P.one_minus_alpha, expf(-__fmul_rn(P.gamma, softplus(-x))));
  if (!GRAD) return __fmul_rn(mod, softplus(x));
  const float inner = __fadd_rn(__fmul_rn(__fmul_rn(P.gamma, sigmoid(-x)), softplus(x)), sigmoid(x));
  return __fmul_rn(mod, inner);
}

// Balanced L1 (Libra R-CNN) of one box coordinate, knee at beta:
//   a <  beta:  t = log1pf((b a) / beta);  l = ((alpha / b) (b a + 1)) t - alpha a
//               dl = sign(d) (alpha t + (alpha (1 - beta)) / (b a + beta))
//   a >= beta:  l = gamma a + (gamma / b - alpha beta);                              dl = sign(d) gamma
// d = pred - target, a = |d|; b = e^(gamma / alpha) - 1 and the constants alpha / b, gamma / b - alpha beta and
// alpha (1 - beta) are formed on the host in double and rounded once.  The second term of dl is what the derivative of l
// has beside alpha t when the knee is not at 1; at beta = 1 it is +0 and dl = sign(d) (alpha t) bit for bit.
// a = 0 gives loss 0 and gradient 0 exactly (sign(0) = 0); a == beta is the outer branch.
struct BalancedL1 {
  float alpha, gamma, beta, b, alpha_over_b, outer_c, knee_c;
};
template <bool GRAD>
__device__ __forceinline__ float balanced_l1(float pred, float target, const BalancedL1& P) {
  const float d = __fsub_rn(pred, target);
  const float a = fabsf(d);
  if (a < P.beta) {
    const float ba = __fmul_rn(P.b, a);
    const float t = log1pf(__fdiv_rn(ba, P.beta));
    if (GRAD) {
      const float v = __fadd_rn(__fmul_rn(P.alpha, t), __fdiv_rn(P.knee_c, __fadd_rn(ba, P.beta)));
      return d > 0.f ? v : (d < 0.f ? -v : d);
    }
    return __fsub_rn(__fmul_rn(__fmul_rn(P.alpha_over_b, __fadd_rn(ba, 1.f)), t), __fmul_rn(P.alpha, a));
  }
  if (GRAD) return d > 0.f ? P.gamma : (d < 0.f ? -P.gamma : d);      // NaN stays NaN
  return __fadd_rn(__fmul_rn(P.gamma, a), P.outer_c);
}

// ---- storage types ------------------------------------------------------------------------------------------------
template <int DT> struct Elem;
template <> struct Elem<TDN_F32> {
  typedef float T;
  static constexpr int V = 4;
  static __device__ __forceinline__ float ld(T v) { return v; }
  static __device__ __forceinline__ T st(float v) { return v; }
};
template <> struct Elem<TDN_BF16> {
  typedef bf16_t T;
  static constexpr int V = 8;
  static __device__ __forceinline__ float ld(T v) { return (float)v; }
  static __device__ __forceinline__ T st(float v) { return (bf16_t)v; }
};
template <> struct Elem<TDN_F16> {
  typedef f16_t T;
  static constexpr int V = 8;
  static __device__ __forceinline__ float ld(T v) { return (float)v; }
  static __device__ __forceinline__ T st(float v) { return (f16_t)v; }
};

template <typename T, int V>
struct alignas(16) Vec {
  T v[V];
};

// ---- xor tree over the lanes of a wavefront ------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
