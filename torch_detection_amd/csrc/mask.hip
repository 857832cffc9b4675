// The mask branch of Mask R-CNN (gfx950; DESIGN.md §4g has the spec, tests/mask_ref.py restates it): polygon mask
// targets, the mask loss with its gradient, rois from detections and the paste of predicted masks into a canvas.
//
// Per-element work is fp32 with explicit __f*_rn arithmetic (this file is compiled with -ffp-contract=off); the loss is
// summed in fp64 in an order fixed by the shapes: a workgroup's partial goes to the workspace with a plain store and the
// last launch adds the partials in index order.  A row whose weight is exactly 0 is never read.  Every output byte is
// written exactly once, zeros included.  No float atomics, no memset, no host synchronisation, no allocation; every
// launch goes through TDN_LAUNCH.
#include "common.h"
#include <string.h>

namespace {

constexpr int MAXM = TDN_MASK_MAX_SIZE;
constexpr int MAXMM = MAXM * MAXM;

// ---- elementwise spec (§4e's e, sp, σ) ------------------------------------------------------------------------------
__device__ __forceinline__ float e_neg_abs(float z) { return expf(-fabsf(z)); }
__device__ __forceinline__ float softplus(float z) { return __fadd_rn(fmaxf(z, 0.f), log1pf(e_neg_abs(z))); }
__device__ __forceinline__ float sigmoid(float z) {
  const float e = e_neg_abs(z);
  const float d = __fadd_rn(1.f, e);
  return z >= 0.f ? __fdiv_rn(1.f, d) : __fdiv_rn(e, d);
}

// truncation toward zero, saturating at the ends of int32; NaN -> 0
__device__ __forceinline__ int trunc_sat(float v) {
  if (!(v == v)) return 0;
  if (v >= 2147483648.f) return 2147483647;
  if (v <= -2147483648.f) return -2147483647 - 1;
  return (int)v;
}
// §4c step 1: the truncated batch index is in [0, B) (NaN is not)
__device__ __forceinline__ bool row_batch(float bf, int B, int* b) {
  if (!(bf > -1.f && bf < (float)B)) return false;
  *b = (int)bf;
  return true;
}
// the box of a row as integers: x1, y1 and w = max(x2 - x1 + 1, 1), h alike
struct IBox {
  int x1, y1;
  long long w, h;
};
__device__ __forceinline__ IBox int_box(const float* c) {
  IBox b;
  b.x1 = trunc_sat(c[0]);
  b.y1 = trunc_sat(c[1]);
  b.w = (long long)trunc_sat(c[2]) - b.x1 + 1;
  b.h = (long long)trunc_sat(c[3]) - b.y1 + 1;
  b.w = b.w > 1 ? b.w : 1;
  b.h = b.h > 1 ? b.h : 1;
  return b;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

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

// element (r, c, p) of a (R, C, M, M) tensor in either memory order
__device__ __forceinline__ size_t pred_index(int nhwc, size_t r, int c, int p, int C, int MM) {
  return nhwc ? (r * MM + p) * C + c : (r * C + c) * MM + p;
}
// the channel a row reads: its label in 1..C-1, or channel 0 of a class-agnostic head
__device__ __forceinline__ bool row_channel(long long lab, int C, int* ch) {
  if (C == 1) {
    *ch = 0;
    return true;
  }
  if (lab < 1 || lab >= C) return false;
  *ch = (int)lab;
  return true;
}

// ---- mask targets ---------------------------------------------------------------------------------------------------
// One workgroup per row.  Thread t owns cells t, t + 256, ...: their centres and one parity bit each stay in registers.
// The instance's polygons are walked one at a time, their vertices staged through LDS 512 at a time (plus the vertex
// that closes the chunk's last edge); the edge loop is uniform, every lane reads the same two vertices.
constexpr int TT = 256;
constexpr int TCH = 512;
constexpr int TK = (MAXMM + TT - 1) / TT;

__global__ __launch_bounds__(TT) void mask_target_kernel(const float* __restrict__ rois, const int32_t* __restrict__ gt_inds,
                                                         const float* __restrict__ poly_xy, int P,
                                                         const int32_t* __restrict__ poly_off, int Q,
                                                         const int32_t* __restrict__ gt_poly_off, int B, int G, int M,
                                                         uint8_t* __restrict__ targets, float* __restrict__ weights) {
  __shared__ float vx[TCH + 1], vy[TCH + 1];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int MM = M * M;
  const int kmax = (MM + TT - 1) / TT;
  const float* row = rois + (size_t)r * 5;
  uint8_t* out = targets + (size_t)r * MM;
  int b = 0;
  const int g = gt_inds[r];
  if (!row_batch(row[0], B, &b) || g < 0 || g >= G) {                // uniform
    for (int c = tid; c < MM; c += TT) out[c] = 0;
    if (tid == 0) weights[r] = 0.f;
    return;
  }
  const IBox bx = int_box(row + 1);
  const float x1f = (float)bx.x1, y1f = (float)bx.y1, wf = (float)bx.w, hf = (float)bx.h, Mf = (float)M;
  float px[TK], py[TK];
#pragma unroll
  for (int k = 0; k < TK; ++k) {
    const int c = tid + k * TT;
    const int i = c / M, j = c - i * M;
    px[k] = __fadd_rn(x1f, __fdiv_rn(__fmul_rn(__fadd_rn((float)j, 0.5f), wf), Mf));
    py[k] = __fadd_rn(y1f, __fdiv_rn(__fmul_rn(__fadd_rn((float)i, 0.5f), hf), Mf));
  }
  unsigned inside = 0;
  const int32_t* go = gt_poly_off + (size_t)b * (G + 1) + g;
  const int q0 = clampi(go[0], 0, Q), q1 = clampi(go[1], 0, Q);
  for (int q = q0; q < q1; ++q) {
    const int s = clampi(poly_off[q], 0, P), e = clampi(poly_off[q + 1], 0, P);
    const int n = e - s;
    if (n < 3) continue;
    unsigned par = 0;
    for (int c0 = 0; c0 < n; c0 += TCH) {
      const int cnt = n - c0 < TCH ? n - c0 : TCH;
      __syncthreads();
      for (int j = tid; j <= cnt; j += TT) {
        const int v = c0 + j;
        const float* p = poly_xy + (size_t)(v < n ? s + v : s) * 2;
        vx[j] = p[0];
        vy[j] = p[1];
      }
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        const float xa = vx[j], ya = vy[j], xb = vx[j + 1], yb = vy[j + 1];
        const float dx = __fsub_rn(xb, xa), dy = __fsub_rn(yb, ya);
#pragma unroll
        for (int k = 0; k < TK; ++k) {
          if (k < kmax && ((ya > py[k]) != (yb > py[k]))) {
            const float xi = __fadd_rn(xa, __fdiv_rn(__fmul_rn(__fsub_rn(py[k], ya), dx), dy));
            if (px[k] < xi) par ^= 1u << k;
          }
        }
      }
    }
    inside |= par;
  }
#pragma unroll
  for (int k = 0; k < TK; ++k) {
    const int c = tid + k * TT;
    if (c < MM) out[c] = (uint8_t)((inside >> k) & 1u);
  }
  if (tid == 0) weights[r] = 1.f;
}

// ---- mask loss ------------------------------------------------------------------------------------------------------
constexpr int LT = 256;            // threads per workgroup
constexpr int LWAVES = LT / 64;
constexpr int LMAX_BLOCKS = 256;   // partials for the last launch
constexpr int PART = 2;            // doubles per partial: the loss sum, rows with weight > 0

struct LossArgs {
  const void* pred;
  void* dpred;
  const uint8_t* targets;
  const int64_t* labels;
  const float* w;
  int32_t R, C, M, nhwc;
  uint32_t n, nchunks;             // backward: elements, 16-byte chunks
  int32_t vec;                     // backward: dpred is 16-byte aligned
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One workgroup per row and grid stride; thread t takes elements t, t + 256, ... of the row's channel.
template <int DT>
__global__ __launch_bounds__(LT) void mask_loss_fwd_kernel(const LossArgs A, double* __restrict__ partials) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ double red[LWAVES][PART];
  const int MM = A.M * A.M;
  double acc = 0.0, cnt = 0.0;
  for (int r = blockIdx.x; r < A.R; r += gridDim.x) {
    const float w = A.w[r];
    if (threadIdx.x == 0 && w > 0.f) cnt += 1.0;
    if (w == 0.f) continue;                                          // uniform
    int ch = 0;
    if (!row_channel(A.labels[r], A.C, &ch)) continue;
    const uint8_t* t = A.targets + (size_t)r * MM;
    for (int p = threadIdx.x; p < MM; p += LT) {
      const float x = E::ld(((const T*)A.pred)[pred_index(A.nhwc, r, ch, p, A.C, MM)]);
      const float l = t[p] ? softplus(-x) : softplus(x);
      acc += (double)__fmul_rn(w, l);
    }
  }
  acc = wave_sum(acc);
  cnt = wave_sum(cnt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = acc;
    red[wave][1] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int v = 0; v < LWAVES; ++v) {
      s0 += red[v][0];
      s1 += red[v][1];
    }
    partials[(size_t)blockIdx.x * PART + 0] = s0;
    partials[(size_t)blockIdx.x * PART + 1] = s1;
  }
}

struct AvgArgs {
  const int32_t* a;
  const int32_t* b;
  int32_t na, nb, mode;
  float value;
};

__global__ __launch_bounds__(LMAX_BLOCKS) void mask_loss_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                         const AvgArgs V, int MM, float* __restrict__ loss,
                                                                         float* __restrict__ avg_out) {
  __shared__ double stage[LMAX_BLOCKS][PART];
  const int t = threadIdx.x;
  if (t < nparts) {
    stage[t][0] = partials[(size_t)t * PART + 0];
    stage[t][1] = partials[(size_t)t * PART + 1];
  }
  __syncthreads();
  if (t != 0) return;
  double s0 = 0.0, s1 = 0.0;
  for (int i = 0; i < nparts; ++i) {
    s0 += stage[i][0];
    s1 += stage[i][1];
  }
  float avg;
  if (V.mode == 0) {
    avg = V.value;
  } else {
    long long n = 0;
    if (V.mode == 1) {
      for (int i = 0; i < V.na; ++i) n += V.a[i];
      for (int i = 0; i < V.nb; ++i) n += V.b[i];
    } else {
      n = (long long)s1;                         // a count of rows: exact in fp64
    }
    avg = (float)(n < 1 ? 1ll : n);
  }
  loss[0] = (float)(s0 / ((double)avg * (double)MM));
  avg_out[0] = avg;
}

// The gradient as the flat array it is in memory, in chunks of 16 bytes; the coordinates of a chunk's first element come
// from two divisions, the following elements advance them.  Only the elements of a live row's channel read the logits.
template <int DT>
__global__ __launch_bounds__(LT) void mask_loss_bwd_kernel(const LossArgs A, const float* __restrict__ g,
                                                           const float* __restrict__ avg) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  const uint32_t MM = (uint32_t)(A.M * A.M), C = (uint32_t)A.C;
  const float s = __fdiv_rn(g[0], __fmul_rn(avg[0], (float)MM));
  for (uint32_t ci = blockIdx.x * (uint32_t)LT + threadIdx.x; ci < A.nchunks; ci += gridDim.x * (uint32_t)LT) {
    const uint32_t m0 = ci * (uint32_t)V;
    const int cnt = (int)min((uint32_t)V, A.n - m0);
    uint32_t r, c, p;
    if (A.nhwc) {
      const uint32_t q = m0 / C;
      c = m0 - q * C;
      r = q / MM;
      p = q - r * MM;
    } else {
      const uint32_t q = m0 / MM;
      p = m0 - q * MM;
      r = q / C;
      c = q - r * C;
    }
    uint32_t last_r = 0xffffffffu;
    float w = 0.f;
    int ch = -1;                                  // the live channel of row last_r, or -1
    Vec<T, V> out;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float res = 0.f;
      if (e < cnt) {
        if (r != last_r) {
          last_r = r;
          w = A.w[r];
          ch = -1;
          if (w != 0.f && !row_channel(A.labels[r], A.C, &ch)) ch = -1;
        }
        if ((int)c == ch) {
          const float x = E::ld(((const T*)A.pred)[m0 + e]);
          const float dl = A.targets[(size_t)r * MM + p] ? -sigmoid(-x) : sigmoid(x);
          res = __fmul_rn(__fmul_rn(w, dl), s);
        }
        if (A.nhwc) {
          if (++c == C) {
            c = 0;
            if (++p == MM) { p = 0; ++r; }
          }
        } else {
          if (++p == MM) {
            p = 0;
            if (++c == C) { c = 0; ++r; }
          }
        }
      }
      out.v[e] = E::st(res);
    }
    T* dp = (T*)A.dpred + m0;
    if (A.vec && cnt == V) {
      *(Vec<T, V>*)dp = out;
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (e < cnt) dp[e] = out.v[e];
    }
  }
}

// ---- rois from detections -------------------------------------------------------------------------------------------
__global__ void rois_from_detections_kernel(const float* __restrict__ dets, const int32_t* __restrict__ counts, int B,
                                            int max_num, const float* __restrict__ scales, float scale,
                                            float* __restrict__ rois) {
  const int64_t total = (int64_t)B * max_num;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / max_num), m = (int)(i % max_num);
    const float* p = dets + i * 5;
    float* o = rois + i * 5;
    if (m < counts[b]) {
      const float s = scales ? scales[b] : scale;
      o[0] = (float)b;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e + 1] = __fmul_rn(p[e], s);
    } else {
      o[0] = -1.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e + 1] = 0.f;
    }
  }
}

// ---- mask paste -----------------------------------------------------------------------------------------------------
// One workgroup per (detection, 16 canvas rows).  A workgroup whose rows meet the clipped box computes the detection's
// M x M probabilities once into LDS; the others only store zeros.  Unpacked: wave v takes rows v, v + 4, .. of the
// tile, a lane computes 4 neighbouring pixels and stores them as one word where the address allows.  Packed: the tile's
// words are one contiguous range and a lane owns one 64-pixel word; the words that meet the box are evaluated one after
// the other by the whole wavefront, a pixel per lane, and the ballot goes to the word's owner; then every lane stores
// its word, 512 contiguous bytes per wavefront.
constexpr int PT = 256;
constexpr int PTH = 16;

struct PasteArgs {
  const void* pred;
  const float* dets;
  const int64_t* labels;
  const int32_t* counts;
  const int32_t* img_shapes;
  uint8_t* out;
  int32_t max_num, C, M, nhwc, H, W, tiles, PW;      // PW: bytes per packed row
  float thr;
};

// one axis of the sample at canvas offset `off` from the box's first pixel (§4c step 5's axis on an M-wide map)
struct PAxis {
  int lo, hi;
  float l, h;
};
__device__ __forceinline__ PAxis paste_axis(long long off, float Mf, float extent, int M) {
  PAxis a;
  float s = __fsub_rn(__fdiv_rn(__fmul_rn(__fadd_rn((float)off, 0.5f), Mf), extent), 0.5f);
  s = s > 0.f ? s : 0.f;
  a.lo = (int)s;                                   // s < M
  if (a.lo >= M - 1) {
    a.lo = a.hi = M - 1;
    a.l = 0.f;
  } else {
    a.hi = a.lo + 1;
    a.l = __fsub_rn(s, (float)a.lo);
  }
  a.h = __fsub_rn(1.f, a.l);
  return a;
}

// the clipped box [xa, xb) x [ya, yb) of a detection and what its samples need
struct PasteBox {
  int xa, xb, ya, yb, x1, y1, M;
  float wf, hf, Mf, thr;
};
// pixel (x, y) of the clipped box: the interpolated probability against the threshold
__device__ __forceinline__ bool paste_pixel(const float* prob, const PasteBox& P, const PAxis& ay, int x) {
  const PAxis ax = paste_axis((long long)x - P.x1, P.Mf, P.wf, P.M);
  const float* p_lo = prob + ay.lo * P.M;
  const float* p_hi = prob + ay.hi * P.M;
  const float w1 = __fmul_rn(ay.h, ax.h), w2 = __fmul_rn(ay.h, ax.l), w3 = __fmul_rn(ay.l, ax.h),
              w4 = __fmul_rn(ay.l, ax.l);
  const float v = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, p_lo[ax.lo]), __fmul_rn(w2, p_lo[ax.hi])),
                                      __fmul_rn(w3, p_hi[ax.lo])),
                            __fmul_rn(w4, p_hi[ax.hi]));
  return v > P.thr;
}

template <int DT, bool PACKED>
__global__ __launch_bounds__(PT) void mask_paste_kernel(const PasteArgs A) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ float prob[MAXMM];
  const int n = blockIdx.x / A.tiles, tile = blockIdx.x - n * A.tiles;
  const int b = n / A.max_num, d = n - b * A.max_num;
  const int M = A.M, MM = M * M, H = A.H, W = A.W;
  const int ty0 = tile * PTH, ty1 = min(ty0 + PTH, H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // everything up to the barrier is uniform
  bool live = d < A.counts[b];
  int ch = 0;
  if (live && A.C > 1) {
    const long long lab = A.labels[n];
    live = lab >= 0 && lab < A.C - 1;
    ch = (int)lab + 1;
  }
  PasteBox P = {0, 0, 0, 0, 0, 0, M, 1.f, 1.f, (float)M, A.thr};
  if (live) {
    int LH = H, LW = W;
    if (A.img_shapes) {
      LH = clampi(A.img_shapes[b * 2 + 0], 0, H);
      LW = clampi(A.img_shapes[b * 2 + 1], 0, W);
    }
    const IBox bx = int_box(A.dets + (size_t)n * 5);
    const long long ex = (long long)bx.x1 + bx.w, ey = (long long)bx.y1 + bx.h;
    P.x1 = bx.x1;
    P.y1 = bx.y1;
    P.wf = (float)bx.w;
    P.hf = (float)bx.h;
    P.xa = bx.x1 > 0 ? bx.x1 : 0;
    P.ya = bx.y1 > 0 ? bx.y1 : 0;
    P.xb = (int)(ex < LW ? (ex > 0 ? ex : 0) : LW);
    P.yb = (int)(ey < LH ? (ey > 0 ? ey : 0) : LH);
    live = P.xa < P.xb && max(P.ya, ty0) < min(P.yb, ty1);
  }
  if (live) {
    for (int m = threadIdx.x; m < MM; m += PT)
      prob[m] = sigmoid(E::ld(((const T*)A.pred)[pred_index(A.nhwc, (size_t)n, ch, m, A.C, MM)]));
    __syncthreads();
  }
  if (PACKED) {
    const int wpr = A.PW >> 3;                                   // 64-pixel words per row
    const int nwords = (ty1 - ty0) * wpr;
    unsigned long long* base = (unsigned long long*)(A.out + ((size_t)n * H + ty0) * A.PW);
    for (int w0 = wave * 64; w0 < nwords; w0 += PT) {            // uniform per wavefront
      const int wi = w0 + lane;
      const int y = ty0 + wi / wpr, x0 = (wi - (y - ty0) * wpr) * 64;
      const bool meets = live && wi < nwords && y >= P.ya && y < P.yb && x0 < P.xb && x0 + 64 > P.xa;
      unsigned long long todo = __ballot(meets), word = 0;
      while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int yj = ty0 + (w0 + j) / wpr, xj = ((w0 + j) - (yj - ty0) * wpr) * 64 + lane;
        const PAxis ay = paste_axis((long long)yj - P.y1, P.Mf, P.hf, M);
        const unsigned long long bits = __ballot(xj >= P.xa && xj < P.xb && paste_pixel(prob, P, ay, xj));
        if (lane == j) word = bits;
      }
      if (wi < nwords) base[wi] = word;
    }
  } else {
    for (int y = ty0 + wave; y < ty1; y += PT / 64) {
      const bool rowlive = live && y >= P.ya && y < P.yb;        // uniform per wavefront
      PAxis ay = {0, 0, 0.f, 1.f};
      if (rowlive) ay = paste_axis((long long)y - P.y1, P.Mf, P.hf, M);
      uint8_t* orow = A.out + ((size_t)n * H + y) * W;
      for (int x0 = lane * 4; x0 < W; x0 += 64 * 4) {
        uint32_t word = 0;
        if (rowlive) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = x0 + e;
            if (x >= P.xa && x < P.xb && paste_pixel(prob, P, ay, x)) word |= 1u << (8 * e);
          }
        }
        if (x0 + 4 <= W && (((uintptr_t)(orow + x0)) & 3) == 0) {
          *(uint32_t*)(orow + x0) = word;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (x0 + e < W) orow[x0 + e] = (uint8_t)((word >> (8 * e)) & 0xffu);
        }
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct PartialsWs { double* partials; int64_t bytes; };
PartialsWs partials_layout(int blocks, void* base) {
  tdn_carver c{(char*)base, 0};
  return {c.take<double>((int64_t)blocks * PART), c.off};
}

int loss_blocks(int R) { return R < 1 ? 1 : (R < LMAX_BLOCKS ? R : LMAX_BLOCKS); }

bool dtype_ok(int dtype) { return dtype == TDN_F32 || dtype == TDN_BF16 || dtype == TDN_F16; }

int check_avg(const char* who, const tdn_loss_avg* avg, AvgArgs* out) {
  TDN_CHECK(avg != nullptr, "%s: NULL avg", who);
  TDN_CHECK(avg->mode == 0 || avg->mode == 1 || avg->mode == 2, "%s: avg mode %d", who, avg->mode);
  if (avg->mode == 0) TDN_CHECK(avg->value > 0.f && avg->value < INFINITY, "%s: avg value must be finite and > 0", who);
  if (avg->mode == 1) {
    TDN_CHECK(avg->na >= 0 && avg->na <= TDN_LOSS_MAX_AVG && avg->nb >= 0 && avg->nb <= TDN_LOSS_MAX_AVG,
              "%s: an avg tensor has more than %d elements", who, TDN_LOSS_MAX_AVG);
    TDN_CHECK((avg->na == 0 || avg->a) && (avg->nb == 0 || avg->b), "%s: NULL avg tensor", who);
  }
  out->a = avg->a;
  out->b = avg->b;
  out->na = avg->mode == 1 ? avg->na : 0;
  out->nb = avg->mode == 1 ? avg->nb : 0;
  out->mode = avg->mode;
  out->value = avg->value;
  return 0;
}

int check_pred(const char* who, int dtype, int64_t R, int C, int M) {
  TDN_CHECK(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  TDN_CHECK(R >= 0 && R <= TDN_LOSS_MAX_ROWS, "%s: R=%lld out of 0..%d", who, (long long)R, TDN_LOSS_MAX_ROWS);
  TDN_CHECK(C >= 1 && C <= TDN_LOSS_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_LOSS_MAX_CLASSES);
  TDN_CHECK(M >= 1 && M <= MAXM, "%s: M=%d out of 1..%d", who, M, MAXM);
  TDN_CHECK(R * C * M * M < (1ll << 31), "%s: the predictions hold 2^31 elements or more", who);
  return 0;
}

#define MASK_LAUNCH_DT(kernel, dtype, grid, block, st, ...)                                 \
  do {                                                                                      \
    if ((dtype) == TDN_F32) TDN_LAUNCH((kernel<TDN_F32>), grid, block, 0, st, __VA_ARGS__); \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((kernel<TDN_F16>), grid, block, 0, st, __VA_ARGS__); \
    else TDN_LAUNCH((kernel<TDN_BF16>), grid, block, 0, st, __VA_ARGS__);                   \
  } while (0)
#define PASTE_LAUNCH_DT(PACKED, dtype, grid, st, ...)                                                            \
  do {                                                                                                           \
    if ((dtype) == TDN_F32) TDN_LAUNCH((mask_paste_kernel<TDN_F32, PACKED>), grid, dim3(PT), 0, st, __VA_ARGS__); \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((mask_paste_kernel<TDN_F16, PACKED>), grid, dim3(PT), 0, st, __VA_ARGS__); \
    else TDN_LAUNCH((mask_paste_kernel<TDN_BF16, PACKED>), grid, dim3(PT), 0, st, __VA_ARGS__);                  \
  } while (0)

}  // namespace

extern "C" int tdn_mask_target(const float* rois, const int32_t* gt_inds, int R, const float* poly_xy, int P,
                               const int32_t* poly_offsets, int Q, const int32_t* gt_poly_offsets, int B, int G, int M,
                               uint8_t* targets, float* weights, void* stream) {
  const char* who = "tdn_mask_target";
  TDN_CHECK(R >= 0 && R <= TDN_LOSS_MAX_ROWS, "%s: R=%d out of 0..%d", who, R, TDN_LOSS_MAX_ROWS);
  TDN_CHECK(M >= 1 && M <= MAXM, "%s: M=%d out of 1..%d", who, M, MAXM);
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(G >= 0 && G <= TDN_TARGET_MAX_GT, "%s: G=%d out of 0..%d", who, G, TDN_TARGET_MAX_GT);
  TDN_CHECK(P >= 0 && Q >= 0, "%s: negative polygon counts", who);
  if (R == 0) return 0;
  TDN_CHECK(rois && gt_inds && targets && weights && poly_offsets && gt_poly_offsets && (P == 0 || poly_xy),
            "%s: NULL pointer", who);
  TDN_LAUNCH(mask_target_kernel, dim3(R), dim3(TT), 0, stream, rois, gt_inds, poly_xy, P, poly_offsets, Q,
             gt_poly_offsets, B, G, M, targets, weights);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_mask_loss_workspace_bytes(int R) {
  if (R < 0 || R > TDN_LOSS_MAX_ROWS) {
    tdn_set_error("tdn_mask_loss_workspace_bytes: R=%d out of 0..%d", R, TDN_LOSS_MAX_ROWS);
    return -1;
  }
  return partials_layout(loss_blocks(R), nullptr).bytes;
}

extern "C" int tdn_mask_loss_fwd(const void* pred, int dtype, int nhwc, int R, int C, int M, const uint8_t* targets,
                                 const int64_t* labels, const float* weights, const tdn_loss_avg* avg, float* loss,
                                 float* avg_out, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_mask_loss_fwd";
  AvgArgs V;
  if (check_pred(who, dtype, R, C, M) != 0 || check_avg(who, avg, &V) != 0) return -1;
  TDN_CHECK(loss && avg_out && workspace, "%s: NULL pointer", who);
  TDN_CHECK(R == 0 || (pred && targets && labels && weights), "%s: NULL pointer", who);
  const int blocks = loss_blocks(R);
  const PartialsWs w = partials_layout(blocks, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  LossArgs A;
  memset(&A, 0, sizeof(A));
  A.pred = pred;
  A.targets = targets;
  A.labels = labels;
  A.w = weights;
  A.R = R;
  A.C = C;
  A.M = M;
  A.nhwc = nhwc ? 1 : 0;
  MASK_LAUNCH_DT(mask_loss_fwd_kernel, dtype, dim3(blocks), dim3(LT), stream, A, w.partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(mask_loss_finalize_kernel, dim3(1), dim3(LMAX_BLOCKS), 0, stream, (const double*)w.partials, blocks, V,
             M * M, loss, avg_out);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_mask_loss_bwd(const void* pred, int dtype, int nhwc, int R, int C, int M, const uint8_t* targets,
                                 const int64_t* labels, const float* weights, const float* g, const float* avg_in,
                                 void* dpred, void* stream) {
  const char* who = "tdn_mask_loss_bwd";
  if (check_pred(who, dtype, R, C, M) != 0) return -1;
  if (R == 0) return 0;
  TDN_CHECK(pred && targets && labels && weights && g && avg_in && dpred, "%s: NULL pointer", who);
  const int V = dtype == TDN_F32 ? 4 : 8;
  LossArgs A;
  memset(&A, 0, sizeof(A));
  A.pred = pred;
  A.dpred = dpred;
  A.targets = targets;
  A.labels = labels;
  A.w = weights;
  A.R = R;
  A.C = C;
  A.M = M;
  A.nhwc = nhwc ? 1 : 0;
  A.n = (uint32_t)((int64_t)R * C * M * M);
  A.nchunks = (A.n + V - 1) / V;
  A.vec = ((uintptr_t)dpred & 15) == 0;
  MASK_LAUNCH_DT(mask_loss_bwd_kernel, dtype, dim3(tdn_grid_1d(A.nchunks, LT, 4096)), dim3(LT), stream, A, g, avg_in);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_rois_from_detections(const float* dets, const int32_t* counts, int B, int max_num,
                                        const float* scale_factors, float scale_factor, float* rois, void* stream) {
  const char* who = "tdn_rois_from_detections";
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(max_num >= 1 && max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, max_num, TDN_RPN_MAX_NUM);
  TDN_CHECK(scale_factors || (scale_factor > 0.f && scale_factor < INFINITY), "%s: scale_factor must be finite and > 0",
            who);
  TDN_CHECK(dets && counts && rois, "%s: NULL pointer", who);
  TDN_LAUNCH(rois_from_detections_kernel, dim3(tdn_grid_1d((int64_t)B * max_num, 256, 1024)), dim3(256), 0, stream, dets,
             counts, B, max_num, scale_factors, scale_factor, rois);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_mask_paste(const void* pred, int dtype, int nhwc, int B, int max_num, int C, int M, const float* dets,
                              const int64_t* labels, const int32_t* counts, const int32_t* img_shapes, int H, int W,
                              float thr, int packed, uint8_t* out, void* stream) {
  const char* who = "tdn_mask_paste";
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(max_num >= 1 && max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, max_num, TDN_RPN_MAX_NUM);
  if (check_pred(who, dtype, (int64_t)B * max_num, C, M) != 0) return -1;
  TDN_CHECK(H >= 1 && W >= 1 && H <= (1 << 16) && W <= (1 << 16), "%s: canvas %d x %d out of 1..65536", who, H, W);
  TDN_CHECK(thr == thr, "%s: thr is NaN", who);
  const int tiles = (H + PTH - 1) / PTH;
  const int64_t grid = (int64_t)B * max_num * tiles;
  TDN_CHECK(grid < (1ll << 31), "%s: %lld workgroups", who, (long long)grid);
  TDN_CHECK(pred && dets && labels && counts && out, "%s: NULL pointer", who);
  PasteArgs A;
  memset(&A, 0, sizeof(A));
  A.pred = pred;
  A.dets = dets;
  A.labels = labels;
  A.counts = counts;
  A.img_shapes = img_shapes;
  A.out = out;
  A.max_num = max_num;
  A.C = C;
  A.M = M;
  A.nhwc = nhwc ? 1 : 0;
  A.H = H;
  A.W = W;
  A.tiles = tiles;
  A.PW = 8 * ((W + 63) / 64);
  A.thr = thr;
  if (packed) {
    TDN_CHECK(((uintptr_t)out & 7) == 0, "%s: the packed output must be 8-byte aligned", who);
    PASTE_LAUNCH_DT(true, dtype, dim3((unsigned)grid), stream, A);
  } else {
    PASTE_LAUNCH_DT(false, dtype, dim3((unsigned)grid), stream, A);
  }
  TDN_LAUNCH_CHECK();
  return 0;
}
