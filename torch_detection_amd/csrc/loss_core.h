// The elementwise spec of the sigmoid classification losses, shared by loss.hip and fcos.hip: fp32 with
// explicit __f*_rn arithmetic in the order written (both files are compiled with -ffp-contract=off); with it the storage
// types of the head outputs, the lane reduction of the fp64 sums, and the walk over the head tensors of a pyramid that
// loss.hip's dense kernel and ghm.hip share.
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

// ---- the walk over the head tensors of a dense anchor head (§4e's dense losses, §4v's GHM) -----------------------------
// One segment = one head tensor of one level, walked as the flat array it is in memory, in chunks of V elements
// (16 bytes).  The table goes to the kernel by value.
struct HeadSeg {
  const void* x;
  void* dx;
  uint32_t n;        // elements
  uint32_t nchunks;
  int64_t chunk0;    // index of the segment's first chunk when the chunks of all segments are numbered through
  int32_t Ch, HW;    // channels, H*W
  int32_t nhwc;      // memory order: 0 (b, c, p), 1 (b, p, c)
  int32_t reg;       // 0: class logits, 1: box deltas
  int32_t off;       // index of the level's first anchor within an image
  int32_t vec;       // x (and dx) are 16-byte aligned
  int32_t row;       // GHM: the level's histogram row
  int32_t pad;
};
constexpr int HEAD_MAXSEG = 2 * TDN_LOSS_MAX_LEVELS;

// the chunk's elements; past the segment's end: zeros
template <int DT>
__device__ __forceinline__ Vec<typename Elem<DT>::T, Elem<DT>::V> head_load(const HeadSeg& S, uint32_t m0, int cnt) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  const T* xp = (const T*)S.x + m0;
  Vec<T, V> in;
  if (S.vec && cnt == V) {
    in = *(const Vec<T, V>*)xp;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) in.v[e] = e < cnt ? xp[e] : E::st(0.f);
  }
  return in;
}
template <int DT>
__device__ __forceinline__ void head_store(const HeadSeg& S, uint32_t m0, int cnt,
                                           const Vec<typename Elem<DT>::T, Elem<DT>::V>& out) {
  typedef typename Elem<DT>::T T;
  constexpr int V = Elem<DT>::V;
  T* dp = (T*)S.dx + m0;
  if (S.vec && cnt == V) {
    *(Vec<T, V>*)dp = out;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (e < cnt) dp[e] = out.v[e];
  }
}

// coordinates of an element: image b, channel c = a * div + k (div channels per anchor), position p
struct HeadPos {
  uint32_t b, c, p;
  int a, k;
};
__device__ __forceinline__ HeadPos head_pos(const HeadSeg& S, uint32_t m0, int div) {
  HeadPos P;
  if (S.nhwc) {
    const uint32_t q = m0 / (uint32_t)S.Ch;
    P.c = m0 - q * (uint32_t)S.Ch;
    P.b = q / (uint32_t)S.HW;
    P.p = q - P.b * (uint32_t)S.HW;
  } else {
    const uint32_t q = m0 / (uint32_t)S.HW;
    P.p = m0 - q * (uint32_t)S.HW;
    P.b = q / (uint32_t)S.Ch;
    P.c = q - P.b * (uint32_t)S.Ch;
  }
  P.a = (int)P.c / div;
  P.k = (int)P.c - P.a * div;
  return P;
}
// the next element in memory order
__device__ __forceinline__ void head_next(const HeadSeg& S, int div, HeadPos& P) {
  if (S.nhwc) {
    ++P.c; ++P.k;
    if (P.k == div) { P.k = 0; ++P.a; }
    if (P.c == (uint32_t)S.Ch) {
      P.c = 0; P.a = 0; P.k = 0; ++P.p;
      if (P.p == (uint32_t)S.HW) { P.p = 0; ++P.b; }
    }
  } else {
    ++P.p;
    if (P.p == (uint32_t)S.HW) {
      P.p = 0; ++P.c; ++P.k;
      if (P.k == div) { P.k = 0; ++P.a; }
      if (P.c == (uint32_t)S.Ch) { P.c = 0; P.a = 0; P.k = 0; ++P.b; }
    }
  }
}

// host: the segment table of L levels without its pointers (segment 2 l + k: level l, kind k), after the checks of the
// level sizes.  Returns N, the anchors per image, or -1 with the error set; *total_chunks: the chunks of all segments.
static inline int64_t head_segments(const char* who, const tdn_loss_level* levels, int L, int B, int dtype, int A, int C,
                                    HeadSeg* seg, int64_t* total_chunks) {
  const int V = dtype == TDN_F32 ? 4 : 8;
  int64_t N = 0, chunk = 0;
  int ns = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_loss_level& lv = levels[l];
    TDN_CHECK(lv.H >= 1 && lv.W >= 1, "%s: level %d is %d x %d", who, l, lv.H, lv.W);
    const int64_t HW = (int64_t)lv.H * lv.W;
    for (int k = 0; k < 2; ++k) {
      const int64_t Ch = k ? 4ll * A : (int64_t)A * C;
      const int64_t n = (int64_t)B * Ch * HW;
      TDN_CHECK(n < (1ll << 31), "%s: level %d holds %lld elements (2^31 or more)", who, l, (long long)n);
      HeadSeg& S = seg[ns++];
      S.n = (uint32_t)n;
      S.nchunks = (uint32_t)((n + V - 1) / V);
      S.chunk0 = chunk;
      S.Ch = (int32_t)Ch;
      S.HW = (int32_t)HW;
      S.nhwc = (k ? lv.reg_nhwc : lv.cls_nhwc) ? 1 : 0;
      S.reg = k;
      S.off = (int32_t)N;
      chunk += S.nchunks;
    }
    N += HW * A;
    TDN_CHECK(N <= TDN_LOSS_MAX_ROWS, "%s: more than %d anchors per image", who, TDN_LOSS_MAX_ROWS);
  }
  *total_chunks = chunk;
  return N;
}
// host: each segment's tensors
static inline int head_pointers(const char* who, const tdn_loss_level* levels, int L, bool grad, HeadSeg* seg) {
  for (int l = 0; l < L; ++l) {
    const tdn_loss_level& lv = levels[l];
    TDN_CHECK(lv.cls && lv.reg && (!grad || (lv.dcls && lv.dreg)), "%s: level %d: NULL pointer", who, l);
    for (int k = 0; k < 2; ++k) {
      HeadSeg& S = seg[2 * l + k];
      S.x = k ? lv.reg : lv.cls;
      S.dx = k ? lv.dreg : lv.dcls;
      S.vec = (((uintptr_t)S.x | (grad ? (uintptr_t)S.dx : 0)) & 15) == 0;
    }
  }
  return 0;
}
