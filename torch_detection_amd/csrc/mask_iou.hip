// Mask Scoring R-CNN around the MaskIoUHead's layers (gfx950; DESIGN.md §4s has the spec, tests/ms_rcnn_ref.py restates
// it): the mask-IoU regression target rasterised from the ground-truth polygons, the MSE loss on the positive targets
// with its gradient, and the test-time product of the predicted IoU with the detection score.
//
// Per-element work is fp32 with explicit __f*_rn arithmetic (this file is compiled with -ffp-contract=off); counts are
// integers; the loss is summed in fp64 in an order fixed by the shapes: a workgroup's partial goes to the workspace with
// a plain store and the last launch adds the partials in index order.  A row that is not live is never read.  Every
// output byte is written exactly once, zeros included.  No float atomics, no memset, no host synchronisation, no
// allocation; every launch goes through TDN_LAUNCH.
#include "loss_core.h"
#include <string.h>

namespace {

constexpr int MAXM = TDN_MASK_MAX_SIZE;

// ---- §4g's row rules, restated from mask.hip (the two files must agree bit for bit) ---------------------------------
// truncation toward zero, saturating at the ends of int32; NaN -> 0
__device__ __forceinline__ int trunc_sat(float v) {
  if (!(v == v)) return 0;
  if (v >= 2147483648.f) return 2147483647;
  if (v <= -2147483648.f) return -2147483647 - 1;
  return (int)v;
}
__device__ __forceinline__ bool row_batch(float bf, int B, int* b) {
  if (!(bf > -1.f && bf < (float)B)) return false;
  *b = (int)bf;
  return true;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
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

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- mask-IoU target ------------------------------------------------------------------------------------------------
// One workgroup per row of rois.  The canvas rows between the polygons' lowest and highest vertex are cut into 64-pixel
// words; a thread owns IK words per pass, their parity and union bits in registers.  The polygons are walked one at a
// time, their vertices staged through LDS 512 at a time as mask_target_kernel does; the edge loop is uniform.  For an
// edge that straddles a word's row the crossing xi is §4g's, and the pixels whose centre compares < xi are the prefix
// [0, n): n = trunc(xi) + (trunc(xi) + 0.5 < xi), both exact in fp32 below 2^23, so the toggle is one mask per word.
constexpr int IT = 256;
constexpr int IWAVES = IT / 64;
constexpr int ICH = 512;
constexpr int IK = 4;
constexpr int CANVAS_MAX = TDN_MASK_IOU_MAX_CANVAS;

struct IouArgs {
  const float* rois;
  const int32_t* gt_inds;
  const float* poly_xy;
  const int32_t* poly_off;
  const int32_t* gt_poly_off;
  const void* pred;
  const int64_t* labels;
  const uint8_t* targets;
  const int32_t* img_shapes;
  float* iou;
  int32_t P, Q, B, G, C, M, nhwc;
  float thr;
};

// pixels x in [0, W) whose centre x + 0.5f compares < xi: a prefix, its length
__device__ __forceinline__ int prefix_len(float xi, int W) {
  if (!(xi > 0.5f)) return 0;                      // NaN too
  if (xi >= (float)W) return W;
  const int t = (int)xi;                           // 0 .. W - 1
  return t + (__fadd_rn((float)t, 0.5f) < xi ? 1 : 0);
}
__device__ __forceinline__ unsigned long long low_bits(int k) {   // k <= 0: none, k >= 64: all
  return k <= 0 ? 0ull : (k >= 64 ? ~0ull : ((1ull << k) - 1ull));
}

template <int DT>
__global__ __launch_bounds__(IT) void mask_iou_target_kernel(const IouArgs A) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ float vx[ICH + 1], vy[ICH + 1];
  __shared__ float ext[IWAVES][2];
  __shared__ int red[IWAVES][5];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = A.M, MM = M * M;
  const float* row = A.rois + (size_t)r * 5;
  int b = 0, ch = 0;
  const int g = A.gt_inds[r];
  if (!row_batch(row[0], A.B, &b) || g < 0 || g >= A.G || !row_channel(A.labels[r], A.C, &ch)) {   // uniform
    if (tid == 0) A.iou[r] = 0.f;
    return;
  }
  const int h = clampi(A.img_shapes[b * 2 + 0], 0, CANVAS_MAX), w = clampi(A.img_shapes[b * 2 + 1], 0, CANVAS_MAX);
  // numpy's y1:y2+1, x1:x2+1 on the canvas (an empty range counts nothing)
  const int bx1 = max(trunc_sat(row[1]), 0), by1 = max(trunc_sat(row[2]), 0);
  const int bx2 = min(trunc_sat(row[3]), w - 1), by2 = min(trunc_sat(row[4]), h - 1);

  // the prediction against the target: pa, ov, ts
  int pa = 0, ov = 0, ts = 0;
  {
    const uint8_t* t = A.targets + (size_t)r * MM;
    for (int p = tid; p < MM; p += IT) {
      const float x = E::ld(((const T*)A.pred)[pred_index(A.nhwc, (size_t)r, ch, p, A.C, MM)]);
      const int on = x > A.thr ? 1 : 0, tv = t[p] == 1 ? 1 : 0;
      pa += on;
      ts += tv;
      ov += on & tv;
    }
  }

  // the y-extent of the instance's vertices (NaN is ignored: an edge with a NaN end toggles nothing)
  const int32_t* go = A.gt_poly_off + (size_t)b * (A.G + 1) + g;
  const int q0 = clampi(go[0], 0, A.Q), q1 = clampi(go[1], 0, A.Q);
  float vmin = INFINITY, vmax = -INFINITY;
  for (int q = q0; q < q1; ++q) {
    const int s = clampi(A.poly_off[q], 0, A.P), e = clampi(A.poly_off[q + 1], 0, A.P);
    for (int v = s + tid; v < e; v += IT) {
      const float y = A.poly_xy[(size_t)v * 2 + 1];
      vmin = fminf(vmin, y);
      vmax = fmaxf(vmax, y);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    vmin = fminf(vmin, __shfl_xor(vmin, o));
    vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  }
  if (lane == 0) {
    ext[wave][0] = vmin;
    ext[wave][1] = vmax;
  }
  __syncthreads();
  vmin = fminf(fminf(ext[0][0], ext[1][0]), fminf(ext[2][0], ext[3][0]));
  vmax = fmaxf(fmaxf(ext[0][1], ext[1][1]), fmaxf(ext[2][1], ext[3][1]));
  // rows y with some vertex <= y + 0.5 and some vertex > y + 0.5, taken one row wider at both ends
  const int ylo = (int)fminf(fmaxf(__fsub_rn(floorf(vmin), 1.f), 0.f), (float)h);
  const int yhi = (int)fminf(fmaxf(__fadd_rn(ceilf(vmax), 1.f), 0.f), (float)h);       // exclusive
  const int wpr = (w + 63) >> 6;
  const int nitems = yhi > ylo ? (yhi - ylo) * wpr : 0;                                // < 2^20

  int full = 0, in = 0;
  for (int base = 0; base < nitems; base += IT * IK) {                                 // uniform
    float py[IK];
    int x0[IK], yy[IK];
    unsigned long long acc[IK];
#pragma unroll
    for (int k = 0; k < IK; ++k) {
      const int it = base + k * IT + tid;
      const int yr = it / wpr;
      yy[k] = it < nitems ? ylo + yr : -1;
      x0[k] = (it - yr * wpr) * 64;
      py[k] = __fadd_rn((float)(ylo + yr), 0.5f);
      acc[k] = 0ull;
    }
    for (int q = q0; q < q1; ++q) {
      const int s = clampi(A.poly_off[q], 0, A.P), e = clampi(A.poly_off[q + 1], 0, A.P);
      const int n = e - s;
      if (n < 3) continue;
      unsigned long long par[IK];
#pragma unroll
      for (int k = 0; k < IK; ++k) par[k] = 0ull;
      for (int c0 = 0; c0 < n; c0 += ICH) {
        const int cnt = n - c0 < ICH ? n - c0 : ICH;
        __syncthreads();
        for (int j = tid; j <= cnt; j += IT) {
          const int v = c0 + j;
          const float* p = A.poly_xy + (size_t)(v < n ? s + v : s) * 2;
          vx[j] = p[0];
          vy[j] = p[1];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
          const float xa = vx[j], ya = vy[j], xb = vx[j + 1], yb = vy[j + 1];
          const float dx = __fsub_rn(xb, xa), dy = __fsub_rn(yb, ya);
#pragma unroll
          for (int k = 0; k < IK; ++k) {
            if (yy[k] >= 0 && ((ya > py[k]) != (yb > py[k]))) {
              const float xi = __fadd_rn(xa, __fdiv_rn(__fmul_rn(__fsub_rn(py[k], ya), dx), dy));
              par[k] ^= low_bits(prefix_len(xi, w) - x0[k]);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < IK; ++k) acc[k] |= par[k];
    }
#pragma unroll
    for (int k = 0; k < IK; ++k) {
      if (yy[k] < 0) continue;
      full += __popcll(acc[k]);
      if (yy[k] >= by1 && yy[k] <= by2) {
        // bits bx1 - x0 .. bx2 - x0 of the word
        const unsigned long long m = low_bits(bx2 - x0[k] + 1) & ~low_bits(bx1 - x0[k]);
        in += __popcll(acc[k] & m);
      }
    }
  }

  int vals[5] = {pa, ov, ts, full, in};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int s = wave_sum_i(vals[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int i = 0; i < 5; ++i) vals[i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
  const float ratio = __fdiv_rn((float)vals[4], __fadd_rn((float)vals[3], 1e-7f));
  const float gf = __fdiv_rn((float)vals[2], __fadd_rn(ratio, 1e-7f));
  const float den = __fsub_rn(__fadd_rn((float)vals[0], gf), (float)vals[1]);
  A.iou[r] = den > 0.f ? __fdiv_rn((float)vals[1], den) : 0.f;
}

// ---- mask-IoU loss --------------------------------------------------------------------------------------------------
constexpr int LT = 256;
constexpr int LWAVES = LT / 64;
constexpr int LMAX_BLOCKS = 256;
constexpr int PART = 2;            // doubles per partial: the sum of squares, the live rows

// row r is live iff its target is > 0 (NaN is not) and its label is in 1..C-1
__device__ __forceinline__ bool iou_live(const float* targets, const int64_t* labels, int r, int C, float* t, int* ch) {
  *t = targets[r];
  if (!(*t > 0.f)) return false;
  const long long lab = labels[r];
  if (lab < 1 || lab >= C) return false;
  *ch = (int)lab;
  return true;
}

template <int DT>
__global__ __launch_bounds__(LT) void mask_iou_loss_fwd_kernel(const void* __restrict__ pred, int R, int C,
                                                               const int64_t* __restrict__ labels,
                                                               const float* __restrict__ targets,
                                                               double* __restrict__ partials) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ double red[LWAVES][PART];
  double acc = 0.0, cnt = 0.0;
  for (int r = blockIdx.x * LT + threadIdx.x; r < R; r += gridDim.x * LT) {
    float t;
    int ch;
    if (!iou_live(targets, labels, r, C, &t, &ch)) continue;
    const float d = __fsub_rn(E::ld(((const T*)pred)[(size_t)r * C + ch]), t);
    acc += (double)__fmul_rn(d, d);
    cnt += 1.0;
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

__global__ __launch_bounds__(LMAX_BLOCKS) void mask_iou_loss_finalize_kernel(const double* __restrict__ partials,
                                                                             int nparts, float loss_weight,
                                                                             float* __restrict__ loss,
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
  const double D = s1 < 1.0 ? 1.0 : s1;            // a count of rows: exact in fp64
  loss[0] = (float)((double)loss_weight * s0 / D);
  avg_out[0] = (float)D;
}

// one thread per element of dpred (R, C)
template <int DT>
__global__ __launch_bounds__(LT) void mask_iou_loss_bwd_kernel(const void* __restrict__ pred, int R, int C,
                                                               const int64_t* __restrict__ labels,
                                                               const float* __restrict__ targets, float two_lw,
                                                               const float* __restrict__ g, const float* __restrict__ avg,
                                                               void* __restrict__ dpred) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const uint32_t n = (uint32_t)R * (uint32_t)C;
  const float s = __fdiv_rn(__fmul_rn(two_lw, g[0]), avg[0]);
  for (uint32_t i = blockIdx.x * (uint32_t)LT + threadIdx.x; i < n; i += gridDim.x * (uint32_t)LT) {
    const uint32_t r = i / (uint32_t)C, c = i - r * (uint32_t)C;
    float res = 0.f, t;
    int ch;
    if (iou_live(targets, labels, (int)r, C, &t, &ch) && (int)c == ch)
      res = __fmul_rn(__fsub_rn(E::ld(((const T*)pred)[i]), t), s);
    ((T*)dpred)[i] = E::st(res);
  }
}

// ---- mask scores ----------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void mask_scores_kernel(const void* __restrict__ pred, int B, int max_num, int C,
                                                          const float* __restrict__ dets,
                                                          const int64_t* __restrict__ labels,
                                                          const int32_t* __restrict__ counts,
                                                          float* __restrict__ scores) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const int total = B * max_num;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int b = i / max_num, d = i - b * max_num;
    float res = 0.f;
    if (d < counts[b]) {
      const long long lab = labels[i];
      if (lab >= -1 && lab < (long long)C - 1)
        res = __fmul_rn(E::ld(((const T*)pred)[(size_t)i * C + (int)(lab + 1)]), dets[(size_t)i * 5 + 4]);
    }
    scores[i] = res;
  }
}

// ---- the mask channel of the MaskIoUHead's first layer --------------------------------------------------------------
// conv(cat(f, P)) = conv_Cf(f) + conv_1(P): the first term is the library's conv launch, the second its epilogue addend,
// formed here.  Forward, one workgroup per row: P = the first maximum of each 2x2 window of sigma(logit) into LDS (and
// to memory with the window index, for the backward), then a[pixel][co] = sum of the nine taps in (ky, kx) order.
constexpr int ST = 256;
constexpr int SWAVES = ST / 64;
constexpr int SMAX = MAXM / 2;
constexpr int STEM_MAX_COUT = TDN_MASK_IOU_MAX_COUT;
constexpr int STEM_MAX_BLOCKS = 256;       // partials of the weight gradient
constexpr uint8_t NO_WINDOW = 255;

// channel of row r for labels[r] + label_offset (the sum wraps instead of overflowing)
__device__ __forceinline__ bool stem_channel(const int64_t* labels, int r, int label_offset, int C, int* ch) {
  return row_channel((long long)((unsigned long long)labels[r] + (unsigned long long)(long long)label_offset), C, ch);
}

struct StemArgs {
  const void* pred;
  const int64_t* labels;
  const float* w1;                 // weight + Cf * 9: element [co][t] at co * wstride + t
  int64_t wstride;
  void* a;
  float* P;
  uint8_t* idx;
  int32_t R, C, S, Cout, nhwc, label_offset;
};

__device__ __forceinline__ void stem_load_w1(float (*ws)[STEM_MAX_COUT], const float* w1, int64_t wstride, int Cout) {
  for (int e = threadIdx.x; e < 9 * Cout; e += ST) {
    const int co = e / 9, t = e - co * 9;
    ws[t][co] = w1[(size_t)co * wstride + t];
  }
}

template <int DT, bool F16>
__global__ __launch_bounds__(ST) void mask_iou_stem_fwd_kernel(const StemArgs A) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ float Ps[SMAX * SMAX];
  __shared__ float ws[9][STEM_MAX_COUT];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int S = A.S, SS = S * S, M = 2 * S, MM = M * M, Cout = A.Cout;
  bf16_t* out = (bf16_t*)A.a + (size_t)r * SS * Cout;
  float* Pg = A.P + (size_t)r * SS;
  uint8_t* ig = A.idx + (size_t)r * SS;
  int ch = 0;
  if (!stem_channel(A.labels, r, A.label_offset, A.C, &ch)) {        // uniform: P = 0, the logits are not read
    const bf16_t z = f32_to_elem<F16>(0.f);
    for (int e = tid; e < SS * Cout; e += ST) out[e] = z;
    for (int p = tid; p < SS; p += ST) {
      Pg[p] = 0.f;
      ig[p] = NO_WINDOW;
    }
    return;
  }
  stem_load_w1(ws, A.w1, A.wstride, Cout);
  for (int p = tid; p < SS; p += ST) {
    const int i = p / S, j = p - i * S;
    float best = 0.f;
    int bi = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int y = 2 * i + (q >> 1), x = 2 * j + (q & 1);
      const float v = sigmoid(E::ld(((const T*)A.pred)[pred_index(A.nhwc, (size_t)r, ch, y * M + x, A.C, MM)]));
      if (q == 0 || v > best) {
        best = v;
        bi = q;
      }
    }
    Ps[p] = best;
    Pg[p] = best;
    ig[p] = (uint8_t)bi;
  }
  __syncthreads();
  for (int e = tid; e < SS * Cout; e += ST) {
    const int p = e / Cout, co = e - p * Cout;
    const int i = p / S, j = p - i * S;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = i + ky - 1, xx = j + kx - 1;
        const float pv = (yy >= 0 && yy < S && xx >= 0 && xx < S) ? Ps[yy * S + xx] : 0.f;
        acc = __fadd_rn(acc, __fmul_rn(ws[ky * 3 + kx][co], pv));
      }
    out[e] = f32_to_elem<F16>(acc);
  }
}

// Backward, first launch.  A workgroup owns a run of pixels (r, i, j).  dP: a wavefront per pixel; per tap the lanes take
// the channels lane, lane + 64, .. in order, an xor tree adds the lanes, the taps are added in (ky, kx) order.  dw1: per
// chunk of 64 channels a lane keeps nine fp64 sums over its wavefront's pixels in order; the four wavefronts are added
// in order and the workgroup's partial goes to the workspace with a plain store.
struct StemBwdArgs {
  const void* gz;
  const float* P;
  const float* w1;
  int64_t wstride;
  float* dP;
  double* partials;
  int32_t S, Cout, npix, ppb;
};

template <bool F16>
__global__ __launch_bounds__(ST) void mask_iou_stem_bwd_kernel(const StemBwdArgs A) {
  __shared__ float ws[9][STEM_MAX_COUT];
  __shared__ double red[SWAVES][9][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = A.S, SS = S * S, Cout = A.Cout;
  const bf16_t* gz = (const bf16_t*)A.gz;
  stem_load_w1(ws, A.w1, A.wstride, Cout);
  __syncthreads();
  const int p0 = blockIdx.x * A.ppb, p1 = min(p0 + A.ppb, A.npix);
  for (int p = p0 + wave; p < p1; p += SWAVES) {
    const int r = p / SS, q = p - r * SS, i = q / S, j = q - i * S;
    float dp = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = i - ky + 1, xx = j - kx + 1;
        if (yy < 0 || yy >= S || xx < 0 || xx >= S) continue;      // uniform per wavefront
        const bf16_t* gp = gz + ((size_t)r * SS + yy * S + xx) * Cout;
        float s = 0.f;
        for (int co = lane; co < Cout; co += 64) s = __fadd_rn(s, __fmul_rn(ws[ky * 3 + kx][co], elem_to_f32<F16>(gp[co])));
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o));
        dp = __fadd_rn(dp, s);
      }
    if (lane == 0) A.dP[p] = dp;
  }
  for (int c0 = 0; c0 < Cout; c0 += 64) {
    double acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.0;
    for (int p = p0 + wave; p < p1; p += SWAVES) {
      const int r = p / SS, q = p - r * SS, i = q / S, j = q - i * S;
      const float gv = elem_to_f32<F16>(gz[(size_t)p * Cout + c0 + lane]);
      const float* Pr = A.P + (size_t)r * SS;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int yy = i + ky - 1, xx = j + kx - 1;
          if (yy >= 0 && yy < S && xx >= 0 && xx < S) acc[ky * 3 + kx] += (double)__fmul_rn(gv, Pr[yy * S + xx]);
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    for (int e = tid; e < 9 * 64; e += ST) {
      const int t = e >> 6, l = e & 63;
      A.partials[((size_t)blockIdx.x * Cout + c0 + l) * 9 + t] = ((red[0][t][l] + red[1][t][l]) + red[2][t][l]) + red[3][t][l];
    }
    __syncthreads();
  }
}

// Backward, second launch.  Workgroups below `nwrite` write dmask_pred as the flat array it is in memory, in chunks of
// 16 bytes (mask_loss_bwd_kernel's walk): the logit that was its window's first maximum gets dP sigma(x) sigma(-x), the
// rest exact zeros.  The workgroups from `nwrite` on add the weight gradient's partials in index order.
struct StemWriteArgs {
  const void* pred;
  void* dpred;
  const int64_t* labels;
  const float* dP;
  const uint8_t* idx;
  const double* partials;
  float* dw1;
  int32_t R, C, S, Cout, nhwc, label_offset, nparts, nwrite;
  uint32_t n, nchunks;
  int32_t vec;
};

template <int DT>
__global__ __launch_bounds__(ST) void mask_iou_stem_write_kernel(const StemWriteArgs A) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  if ((int)blockIdx.x >= A.nwrite) {
    const int e = ((int)blockIdx.x - A.nwrite) * ST + threadIdx.x;
    if (e < A.Cout * 9) {
      double s = 0.0;
      for (int b = 0; b < A.nparts; ++b) s += A.partials[(size_t)b * A.Cout * 9 + e];
      A.dw1[e] = (float)s;
    }
    return;
  }
  const int S = A.S, M = 2 * S;
  const uint32_t MM = (uint32_t)(M * M), C = (uint32_t)A.C, SS = (uint32_t)(S * S);
  for (uint32_t ci = blockIdx.x * (uint32_t)ST + threadIdx.x; ci < A.nchunks; ci += (uint32_t)A.nwrite * (uint32_t)ST) {
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
    int ch = -1;                                  // the live channel of row last_r, or -1
    Vec<T, V> out;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float res = 0.f;
      if (e < cnt) {
        if (r != last_r) {
          last_r = r;
          if (!stem_channel(A.labels, (int)r, A.label_offset, A.C, &ch)) ch = -1;
        }
        if ((int)c == ch) {
          const int y = (int)p / M, x = (int)p - y * M;
          const size_t cell = (size_t)r * SS + (size_t)((y >> 1) * S + (x >> 1));
          if (A.idx[cell] == (uint8_t)(((y & 1) << 1) | (x & 1))) {
            const float xv = E::ld(((const T*)A.pred)[m0 + e]);
            res = __fmul_rn(__fmul_rn(A.dP[cell], sigmoid(xv)), sigmoid(-xv));
          }
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

// ---- host -----------------------------------------------------------------------------------------------------------
struct StemWs { double* partials; int64_t bytes; };
StemWs stem_layout(int blocks, int Cout, void* base) {
  tdn_carver c{(char*)base, 0};
  return {c.take<double>((int64_t)blocks * Cout * 9), c.off};
}
// pixels per workgroup of the first backward launch (a multiple of the wavefronts) and the workgroups
void stem_split(int64_t npix, int* ppb, int* blocks) {
  int64_t per = (npix + STEM_MAX_BLOCKS - 1) / STEM_MAX_BLOCKS;
  per = (per + SWAVES - 1) / SWAVES * SWAVES;
  if (per < SWAVES) per = SWAVES;
  *ppb = (int)per;
  *blocks = (int)((npix + per - 1) / per);
  if (*blocks < 1) *blocks = 1;
}
int check_stem(const char* who, int64_t R, int S, int Cf, int Cout) {
  TDN_CHECK(R >= 1 && R <= TDN_LOSS_MAX_ROWS, "%s: R=%lld out of 1..%d", who, (long long)R, TDN_LOSS_MAX_ROWS);
  TDN_CHECK(S >= 1 && S <= SMAX, "%s: S=%d out of 1..%d", who, S, SMAX);
  TDN_CHECK(Cf >= 64 && Cf % 64 == 0, "%s: Cf=%d must be a positive multiple of 64", who, Cf);
  TDN_CHECK(Cout >= 64 && Cout % 64 == 0 && Cout <= STEM_MAX_COUT, "%s: Cout=%d must be a multiple of 64 in 64..%d", who,
            Cout, STEM_MAX_COUT);
  TDN_CHECK(R * S * S * Cout < (1ll << 31), "%s: the output holds 2^31 elements or more", who);
  return 0;
}

struct PartialsWs { double* partials; int64_t bytes; };
PartialsWs partials_layout(int blocks, void* base) {
  tdn_carver c{(char*)base, 0};
  return {c.take<double>((int64_t)blocks * PART), c.off};
}
int loss_blocks(int R) { return tdn_grid_1d(R, LT, LMAX_BLOCKS); }
bool dtype_ok(int dtype) { return dtype == TDN_F32 || dtype == TDN_BF16 || dtype == TDN_F16; }

int check_rc(const char* who, int dtype, int64_t R, int C) {
  TDN_CHECK(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  TDN_CHECK(R >= 0 && R <= TDN_LOSS_MAX_ROWS, "%s: R=%lld out of 0..%d", who, (long long)R, TDN_LOSS_MAX_ROWS);
  TDN_CHECK(C >= 1 && C <= TDN_LOSS_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_LOSS_MAX_CLASSES);
  return 0;
}

#define MIOU_LAUNCH_DT(kernel, dtype, grid, block, st, ...)                                 \
  do {                                                                                      \
    if ((dtype) == TDN_F32) TDN_LAUNCH((kernel<TDN_F32>), grid, block, 0, st, __VA_ARGS__); \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((kernel<TDN_F16>), grid, block, 0, st, __VA_ARGS__); \
    else TDN_LAUNCH((kernel<TDN_BF16>), grid, block, 0, st, __VA_ARGS__);                   \
  } while (0)

}  // namespace

extern "C" int tdn_mask_iou_target(const float* rois, const int32_t* gt_inds, int R, const float* poly_xy, int P,
                                   const int32_t* poly_offsets, int Q, const int32_t* gt_poly_offsets, int B, int G,
                                   const void* pred, int dtype, int nhwc, int C, int M, const int64_t* labels,
                                   const uint8_t* targets, const int32_t* img_shapes, float thr, float* iou,
                                   void* stream) {
  const char* who = "tdn_mask_iou_target";
  if (check_rc(who, dtype, R, C) != 0) return -1;
  TDN_CHECK(M >= 1 && M <= MAXM, "%s: M=%d out of 1..%d", who, M, MAXM);
  TDN_CHECK((int64_t)R * C * M * M < (1ll << 31), "%s: the predictions hold 2^31 elements or more", who);
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(G >= 0 && G <= TDN_TARGET_MAX_GT, "%s: G=%d out of 0..%d", who, G, TDN_TARGET_MAX_GT);
  TDN_CHECK(P >= 0 && Q >= 0, "%s: negative polygon counts", who);
  TDN_CHECK(thr == thr, "%s: thr is NaN", who);
  if (R == 0) return 0;
  TDN_CHECK(rois && gt_inds && poly_offsets && gt_poly_offsets && (P == 0 || poly_xy) && pred && labels && targets &&
                img_shapes && iou,
            "%s: NULL pointer", who);
  IouArgs A;
  memset(&A, 0, sizeof(A));
  A.rois = rois;
  A.gt_inds = gt_inds;
  A.poly_xy = poly_xy;
  A.poly_off = poly_offsets;
  A.gt_poly_off = gt_poly_offsets;
  A.pred = pred;
  A.labels = labels;
  A.targets = targets;
  A.img_shapes = img_shapes;
  A.iou = iou;
  A.P = P;
  A.Q = Q;
  A.B = B;
  A.G = G;
  A.C = C;
  A.M = M;
  A.nhwc = nhwc ? 1 : 0;
  A.thr = thr;
  MIOU_LAUNCH_DT(mask_iou_target_kernel, dtype, dim3(R), dim3(IT), stream, A);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_mask_iou_loss_workspace_bytes(int R) {
  if (R < 0 || R > TDN_LOSS_MAX_ROWS) {
    tdn_set_error("tdn_mask_iou_loss_workspace_bytes: R=%d out of 0..%d", R, TDN_LOSS_MAX_ROWS);
    return -1;
  }
  return partials_layout(loss_blocks(R), nullptr).bytes;
}

extern "C" int tdn_mask_iou_loss_fwd(const void* pred, int dtype, int R, int C, const int64_t* labels,
                                     const float* targets, float loss_weight, float* loss, float* avg_out,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_mask_iou_loss_fwd";
  if (check_rc(who, dtype, R, C) != 0) return -1;
  TDN_CHECK(loss_weight == loss_weight && loss_weight < INFINITY && loss_weight > -INFINITY, "%s: loss_weight", who);
  TDN_CHECK(loss && avg_out && workspace, "%s: NULL pointer", who);
  TDN_CHECK(R == 0 || (pred && labels && targets), "%s: NULL pointer", who);
  const int blocks = loss_blocks(R);
  const PartialsWs w = partials_layout(blocks, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  MIOU_LAUNCH_DT(mask_iou_loss_fwd_kernel, dtype, dim3(blocks), dim3(LT), stream, pred, R, C, labels, targets,
                 w.partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(mask_iou_loss_finalize_kernel, dim3(1), dim3(LMAX_BLOCKS), 0, stream, (const double*)w.partials, blocks,
             loss_weight, loss, avg_out);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_mask_iou_loss_bwd(const void* pred, int dtype, int R, int C, const int64_t* labels,
                                     const float* targets, float loss_weight, const float* g, const float* avg_in,
                                     void* dpred, void* stream) {
  const char* who = "tdn_mask_iou_loss_bwd";
  if (check_rc(who, dtype, R, C) != 0) return -1;
  TDN_CHECK(loss_weight == loss_weight && loss_weight < INFINITY && loss_weight > -INFINITY, "%s: loss_weight", who);
  if (R == 0) return 0;
  TDN_CHECK(pred && labels && targets && g && avg_in && dpred, "%s: NULL pointer", who);
  MIOU_LAUNCH_DT(mask_iou_loss_bwd_kernel, dtype, dim3(tdn_grid_1d((int64_t)R * C, LT, 4096)), dim3(LT), stream, pred, R,
                 C, labels, targets, 2.f * loss_weight, g, avg_in, dpred);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_mask_scores(const void* pred, int dtype, int B, int max_num, int C, const float* dets,
                               const int64_t* labels, const int32_t* counts, float* scores, void* stream) {
  const char* who = "tdn_mask_scores";
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(max_num >= 1 && max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, max_num, TDN_RPN_MAX_NUM);
  if (check_rc(who, dtype, (int64_t)B * max_num, C) != 0) return -1;
  TDN_CHECK(pred && dets && labels && counts && scores, "%s: NULL pointer", who);
  MIOU_LAUNCH_DT(mask_scores_kernel, dtype, dim3(tdn_grid_1d((int64_t)B * max_num, 256, 1024)), dim3(256), stream, pred,
                 B, max_num, C, dets, labels, counts, scores);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_mask_iou_stem_fwd(const void* pred, int dtype, int nhwc, int R, int C, int S, const int64_t* labels,
                                     int label_offset, const float* weight, int Cf, int Cout, void* a, int out_dtype,
                                     float* P, uint8_t* idx, void* stream) {
  const char* who = "tdn_mask_iou_stem_fwd";
  TDN_CHECK(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  TDN_CHECK_DTYPE(out_dtype);
  TDN_CHECK(C >= 1 && C <= TDN_LOSS_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_LOSS_MAX_CLASSES);
  if (check_stem(who, R, S, Cf, Cout) != 0) return -1;
  TDN_CHECK((int64_t)R * C * 4 * S * S < (1ll << 31), "%s: the predictions hold 2^31 elements or more", who);
  TDN_CHECK(pred && labels && weight && a && P && idx, "%s: NULL pointer", who);
  StemArgs A;
  memset(&A, 0, sizeof(A));
  A.pred = pred;
  A.labels = labels;
  A.w1 = weight + (size_t)Cf * 9;
  A.wstride = ((int64_t)Cf + 1) * 9;
  A.a = a;
  A.P = P;
  A.idx = idx;
  A.R = R;
  A.C = C;
  A.S = S;
  A.Cout = Cout;
  A.nhwc = nhwc ? 1 : 0;
  A.label_offset = label_offset;
  if (out_dtype == TDN_F16) {
    if (dtype == TDN_F32) TDN_LAUNCH((mask_iou_stem_fwd_kernel<TDN_F32, true>), dim3(R), dim3(ST), 0, stream, A);
    else if (dtype == TDN_F16) TDN_LAUNCH((mask_iou_stem_fwd_kernel<TDN_F16, true>), dim3(R), dim3(ST), 0, stream, A);
    else TDN_LAUNCH((mask_iou_stem_fwd_kernel<TDN_BF16, true>), dim3(R), dim3(ST), 0, stream, A);
  } else {
    if (dtype == TDN_F32) TDN_LAUNCH((mask_iou_stem_fwd_kernel<TDN_F32, false>), dim3(R), dim3(ST), 0, stream, A);
    else if (dtype == TDN_F16) TDN_LAUNCH((mask_iou_stem_fwd_kernel<TDN_F16, false>), dim3(R), dim3(ST), 0, stream, A);
    else TDN_LAUNCH((mask_iou_stem_fwd_kernel<TDN_BF16, false>), dim3(R), dim3(ST), 0, stream, A);
  }
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_mask_iou_stem_bwd_workspace_bytes(int R, int S, int Cout) {
  if (check_stem("tdn_mask_iou_stem_bwd_workspace_bytes", R, S, 64, Cout) != 0) return -1;
  int ppb, blocks;
  stem_split((int64_t)R * S * S, &ppb, &blocks);
  return stem_layout(blocks, Cout, nullptr).bytes;
}

extern "C" int tdn_mask_iou_stem_bwd(const void* gz, int gz_dtype, const float* P, const uint8_t* idx, const float* weight,
                                     int Cf, int Cout, const void* pred, int dtype, int nhwc, int R, int C, int S,
                                     const int64_t* labels, int label_offset, float* dP, void* dpred, float* dw1,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_mask_iou_stem_bwd";
  TDN_CHECK(dtype_ok(dtype), "%s: dtype %d", who, dtype);
  TDN_CHECK_DTYPE(gz_dtype);
  TDN_CHECK(C >= 1 && C <= TDN_LOSS_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_LOSS_MAX_CLASSES);
  if (check_stem(who, R, S, Cf, Cout) != 0) return -1;
  TDN_CHECK((int64_t)R * C * 4 * S * S < (1ll << 31), "%s: the predictions hold 2^31 elements or more", who);
  TDN_CHECK(gz && P && idx && weight && pred && labels && dP && dpred && dw1, "%s: NULL pointer", who);
  int ppb, blocks;
  stem_split((int64_t)R * S * S, &ppb, &blocks);
  const StemWs w = stem_layout(blocks, Cout, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  StemBwdArgs Bk;
  memset(&Bk, 0, sizeof(Bk));
  Bk.gz = gz;
  Bk.P = P;
  Bk.w1 = weight + (size_t)Cf * 9;
  Bk.wstride = ((int64_t)Cf + 1) * 9;
  Bk.dP = dP;
  Bk.partials = w.partials;
  Bk.S = S;
  Bk.Cout = Cout;
  Bk.npix = R * S * S;
  Bk.ppb = ppb;
  TDN_LAUNCH_T(mask_iou_stem_bwd_kernel, gz_dtype, dim3(blocks), dim3(ST), stream, Bk);
  TDN_LAUNCH_CHECK();
  const int V = dtype == TDN_F32 ? 4 : 8;
  StemWriteArgs W;
  memset(&W, 0, sizeof(W));
  W.pred = pred;
  W.dpred = dpred;
  W.labels = labels;
  W.dP = dP;
  W.idx = idx;
  W.partials = w.partials;
  W.dw1 = dw1;
  W.R = R;
  W.C = C;
  W.S = S;
  W.Cout = Cout;
  W.nhwc = nhwc ? 1 : 0;
  W.label_offset = label_offset;
  W.nparts = blocks;
  W.n = (uint32_t)((int64_t)R * C * 4 * S * S);
  W.nchunks = (W.n + V - 1) / V;
  W.nwrite = tdn_grid_1d(W.nchunks, ST, 4096);
  W.vec = ((uintptr_t)dpred & 15) == 0;
  const int nfinal = (Cout * 9 + ST - 1) / ST;
  MIOU_LAUNCH_DT(mask_iou_stem_write_kernel, dtype, dim3(W.nwrite + nfinal), dim3(ST), stream, W);
  TDN_LAUNCH_CHECK();
  return 0;
}
