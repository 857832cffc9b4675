// FCOS: the point generator, point-in-box training targets, the focal + IoU + centre-ness loss with its gradients, and
// test-time detections (gfx950; DESIGN.md §4n has the spec, tests/fcos_ref.py restates it).
//
// Semantics are the project's own spec in the mmdetection-v1 lineage (FCOSHead.fcos_target / loss / get_bboxes), '+1'
// boxes, strict IEEE fp32 in the spec's operation order (this file is compiled with -ffp-contract=off).  Points are
// never stored: every kernel recomputes (x, y) = (w*s + s/2, h*s + s/2) from (level, h, w).
// No memset, no atomics on floats, no inter-workgroup waits, no allocation; sums are fp64 (or integer) in an order fixed
// by the shapes, so every output is a pure function of the inputs.
#include "select_core.h"
#include "loss_core.h"
#include <math.h>
#include <string.h>

namespace {

// ---- the pyramid ---------------------------------------------------------------------------------------------------------
struct FcGeo {
  int L, N;
  int off[TDN_FCOS_MAX_LEVELS + 1];            // prefix sums of H*W
  int H[TDN_FCOS_MAX_LEVELS], W[TDN_FCOS_MAX_LEVELS], s[TDN_FCOS_MAX_LEVELS];
  float lo[TDN_FCOS_MAX_LEVELS], hi[TDN_FCOS_MAX_LEVELS];
};

// point i of the pyramid: its level, and through *px / *py its position (exact: integers below 2^24)
__device__ __forceinline__ int fc_locate(const FcGeo& G, int i, float* px, float* py) {
  int l = 0;
  while (l + 1 < G.L && i >= G.off[l + 1]) ++l;
  const int p = i - G.off[l], W = G.W[l], s = G.s[l];
  const int h = p / W, w = p - h * W;
  *px = (float)(w * s + s / 2);
  *py = (float)(h * s + s / 2);
  return l;
}

int fc_geo(const char* who, const tdn_fcos_level* levels, int L, bool ranges, FcGeo* out) {
  TDN_CHECK(levels, "%s: NULL levels", who);
  TDN_CHECK(L >= 1 && L <= TDN_FCOS_MAX_LEVELS, "%s: %d levels (1..%d)", who, L, TDN_FCOS_MAX_LEVELS);
  memset(out, 0, sizeof(*out));
  out->L = L;
  int64_t N = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_fcos_level& v = levels[l];
    TDN_CHECK(v.H >= 1 && v.W >= 1, "%s: level %d is %d x %d", who, l, v.H, v.W);
    TDN_CHECK(v.stride >= 1 && v.stride <= (1 << 15), "%s: level %d has stride %d (1..32768)", who, l, v.stride);
    TDN_CHECK((int64_t)v.H * v.stride < (1 << 24) && (int64_t)v.W * v.stride < (1 << 24),
              "%s: level %d spans 2^24 pixels or more", who, l);
    if (ranges) TDN_CHECK(v.lo <= v.hi, "%s: level %d has no regress range lo <= hi", who, l);   // false for a NaN
    out->off[l] = (int)N;
    out->H[l] = v.H;
    out->W[l] = v.W;
    out->s[l] = v.stride;
    out->lo[l] = v.lo;
    out->hi[l] = v.hi;
    N += (int64_t)v.H * v.W;
    TDN_CHECK(N <= TDN_TARGET_MAX_BOXES, "%s: more than %d points per image", who, TDN_TARGET_MAX_BOXES);
  }
  for (int l = L; l <= TDN_FCOS_MAX_LEVELS; ++l) out->off[l] = (int)N;
  out->N = (int)N;
  return 0;
}

constexpr int FT = 256;

// ---- points --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT) void fcos_points_kernel(const FcGeo G, float* __restrict__ points) {
  const int i = blockIdx.x * FT + threadIdx.x;
  if (i >= G.N) return;
  float x, y;
  const int l = fc_locate(G, i, &x, &y);
  *(f32x4_t*)(points + (int64_t)i * 4) = (f32x4_t){x, y, (float)G.s[l], (float)l};
}

// ---- targets -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float min4(float a, float b, float c, float d) { return fminf(fminf(a, b), fminf(c, d)); }
__device__ __forceinline__ float max4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }

// One thread per (image, point); the image's ground truths and their areas are staged in LDS.  part[b][workgroup] = the
// workgroup's positives, a plain store.
__global__ __launch_bounds__(FT) void fcos_target_kernel(const FcGeo G, const float* __restrict__ gt,
                                                         const int64_t* __restrict__ gt_labels,
                                                         const int32_t* __restrict__ gt_counts, int NG, float rho,
                                                         int64_t* __restrict__ labels, float* __restrict__ bbox_targets,
                                                         int32_t* __restrict__ assigned, int32_t* __restrict__ part) {
  __shared__ f32x4_t sbox[TDN_TARGET_MAX_GT];
  __shared__ float sarea[TDN_TARGET_MAX_GT];
  __shared__ int wpos[FT / 64];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int cnt = NG > 0 ? max(0, min(gt_counts[b], NG)) : 0;
  for (int j = tid; j < cnt; j += FT) {
    const f32x4_t bx = *(const f32x4_t*)(gt + ((int64_t)b * NG + j) * 4);
    sbox[j] = bx;
    sarea[j] = __fmul_rn(__fadd_rn(__fsub_rn(bx[2], bx[0]), 1.f), __fadd_rn(__fsub_rn(bx[3], bx[1]), 1.f));
  }
  __syncthreads();
  const int i = blockIdx.x * FT + tid;
  int pos = 0;
  if (i < G.N) {
    float x, y;
    const int l = fc_locate(G, i, &x, &y);
    const float lo = G.lo[l], hi = G.hi[l];
    const float rs = __fmul_rn(rho, (float)G.s[l]);
    int best = -1;
    float best_area = 0.f;
    f32x4_t t = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < cnt; ++j) {
      const f32x4_t bx = sbox[j];
      const float dl = __fsub_rn(x, bx[0]), dt = __fsub_rn(y, bx[1]), dr = __fsub_rn(bx[2], x),
                  db = __fsub_rn(bx[3], y);
      float inside = min4(dl, dt, dr, db);
      if (rho > 0.f) {
        const float cx = __fmul_rn(__fadd_rn(bx[0], bx[2]), 0.5f), cy = __fmul_rn(__fadd_rn(bx[1], bx[3]), 0.5f);
        const float x1 = fmaxf(__fsub_rn(cx, rs), bx[0]), y1 = fmaxf(__fsub_rn(cy, rs), bx[1]);
        const float x2 = fminf(__fadd_rn(cx, rs), bx[2]), y2 = fminf(__fadd_rn(cy, rs), bx[3]);
        inside = min4(__fsub_rn(x, x1), __fsub_rn(y, y1), __fsub_rn(x2, x), __fsub_rn(y2, y));
      }
      const float far = max4(dl, dt, dr, db);
      const float area = sarea[j];
      if (inside > 0.f && far >= lo && far <= hi && (best < 0 || area < best_area)) {
        best = j;
        best_area = area;
        t = (f32x4_t){dl, dt, dr, db};
      }
    }
    const int64_t q = (int64_t)b * G.N + i;
    labels[q] = best < 0 ? 0 : (gt_labels ? gt_labels[(int64_t)b * NG + best] : 1);
    *(f32x4_t*)(bbox_targets + q * 4) = t;
    assigned[q] = best + 1;
    pos = best >= 0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) pos += __shfl_xor(pos, o);
  if ((tid & 63) == 0) wpos[tid >> 6] = pos;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < FT / 64; ++w) s += wpos[w];
    part[(int64_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// num_pos[b] = the sum of the image's nparts workgroup counts (integers: any order gives the same sum)
__global__ __launch_bounds__(FT) void fcos_count_kernel(const int32_t* __restrict__ part, int nparts,
                                                        int32_t* __restrict__ num_pos) {
  __shared__ int wsum[FT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  int s = 0;
  for (int k = tid; k < nparts; k += FT) s += part[(int64_t)b * nparts + k];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < FT / 64; ++w) tot += wsum[w];
    num_pos[b] = tot;
  }
}

int fc_target_plan(const char* who, const tdn_fcos_level* levels, int L, int B, int NG, FcGeo* G) {
  if (fc_geo(who, levels, L, true, G) != 0) return -1;
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(NG >= 0 && NG <= TDN_TARGET_MAX_GT, "%s: G=%d ground truths per image (max %d)", who, NG, TDN_TARGET_MAX_GT);
  return 0;
}

// ---- loss ----------------------------------------------------------------------------------------------------------------
// One kernel, two walks.  The class logits of every level are walked as the flat arrays they are in memory, in chunks of
// 16 bytes, exactly as loss.hip's dense kernel walks them (focal term, A = 1, every weight 1).  Then, level by level, one
// thread per (image, point): a positive reads its four regression outputs and its centre-ness logit through the
// tensor's layout, everything else reads the label only.  GRAD: the same walks write every gradient element.
constexpr int LT = 1024;            // threads per workgroup: 16 waves, four per SIMD
constexpr int LWAVES = LT / 64;
constexpr int LMAX_BLOCKS = 256;    // that many partials for the last launch
constexpr int FPART = 16;           // doubles per partial
constexpr int P_CLS = 0, P_BOX = 1, P_CSUM = 2, P_CTR = 3, P_NPOS = 4, P_MAIN = 5, P_SCALE = 8;   // .. P_SCALE + L

struct FlSeg {                      // the class logits of one level
  const void* x;
  void* dx;
  uint32_t n, nchunks;              // elements, chunks
  int64_t chunk0;                   // index of the level's first chunk
  int32_t HW, nhwc, off, vec;       // off: the level's first point; vec: x (and dx) are 16-byte aligned
};
struct FlLevel {
  const void* reg;
  const void* ctr;
  void* dreg;
  void* dctr;
  int32_t HW, reg_nhwc;
};
struct FlArgs {
  FlSeg seg[TDN_FCOS_MAX_LEVELS];
  FlLevel lv[TDN_FCOS_MAX_LEVELS];
  int32_t L, B, N, C, giou, has_scales;
  int64_t nchunks;
  const int64_t* labels;
  const float* bt;
  const float* scales;
  float eps;
  ClsParams P;
};

template <int DT, bool GRAD>
__device__ __forceinline__ double fl_cls_chunk(const FlSeg& S, const FlArgs& A, uint32_t lc, float s_cls) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  const uint32_t m0 = lc * (uint32_t)V;
  const int cnt = (int)min((uint32_t)V, S.n - m0);
  const T* xp = (const T*)S.x + m0;
  Vec<T, V> in, out;
  if (S.vec && cnt == V) {
    in = *(const Vec<T, V>*)xp;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) in.v[e] = e < cnt ? xp[e] : E::st(0.f);
  }
  uint32_t b, c, p;                                // coordinates of the chunk's first element
  if (S.nhwc) {
    const uint32_t q = m0 / (uint32_t)A.C;
    c = m0 - q * (uint32_t)A.C;
    b = q / (uint32_t)S.HW;
    p = q - b * (uint32_t)S.HW;
  } else {
    const uint32_t q = m0 / (uint32_t)S.HW;
    p = m0 - q * (uint32_t)S.HW;
    b = q / (uint32_t)A.C;
    c = q - b * (uint32_t)A.C;
  }
  int last_idx = -1;
  long long last_lab = 0;
  double sum = 0.0;                                // the chunk's elements in memory order
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float res = 0.f;
    if (e < cnt) {
      const int idx = (int)b * A.N + S.off + (int)p;               // < 64 * 2^20
      if (idx != last_idx) {
        last_idx = idx;
        last_lab = A.labels[idx];
      }
      const float v = cls_elem<GRAD>(E::ld(in.v[e]), last_lab == (long long)c + 1, A.P);
      if (GRAD) res = __fmul_rn(v, s_cls);
      else sum += (double)v;
      if (S.nhwc) {
        if (++c == (uint32_t)A.C) {
          c = 0;
          if (++p == (uint32_t)S.HW) { p = 0; ++b; }
        }
      } else {
        if (++p == (uint32_t)S.HW) {
          p = 0;
          if (++c == (uint32_t)A.C) { c = 0; ++b; }
        }
      }
    }
    if (GRAD) out.v[e] = E::st(res);
  }
  if (GRAD) {
    T* dp = (T*)S.dx + m0;
    if (S.vec && cnt == V) {
      *(Vec<T, V>*)dp = out;
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (e < cnt) dp[e] = out.v[e];
    }
  }
  return sum;
}

// the box and centre-ness terms of one positive: x = the raw regression outputs, z = the centre-ness logit, t = the
// target distances, s = the level's scale
struct FlPos {
  float c, loss_box, loss_ctr;      // centre-ness target, IoU / GIoU loss, centre-ness BCE
  float e[4];                       // c * dloss/dd_j * d_j
};
template <bool NEED_GRAD>
__device__ __forceinline__ FlPos fl_positive(const float* x, const float* t, float s, int giou, float eps) {
  FlPos R;
  float d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = expf(__fmul_rn(s, x[j]));
  R.c = __fsqrt_rn(__fmul_rn(__fdiv_rn(fminf(t[0], t[2]), fmaxf(t[0], t[2])),
                             __fdiv_rn(fminf(t[1], t[3]), fmaxf(t[1], t[3]))));
  const float wp = __fadd_rn(__fadd_rn(d[0], d[2]), 1.f), hp = __fadd_rn(__fadd_rn(d[1], d[3]), 1.f);
  const float wt = __fadd_rn(__fadd_rn(t[0], t[2]), 1.f), ht = __fadd_rn(__fadd_rn(t[1], t[3]), 1.f);
  const float wi = __fadd_rn(__fadd_rn(fminf(d[0], t[0]), fminf(d[2], t[2])), 1.f);
  const float hi = __fadd_rn(__fadd_rn(fminf(d[1], t[1]), fminf(d[3], t[3])), 1.f);
  const float ap = __fmul_rn(wp, hp), at = __fmul_rn(wt, ht), I = __fmul_rn(wi, hi);
  const float U = __fsub_rn(__fadd_rn(ap, at), I);
  const float iou = __fdiv_rn(I, U);
  float we = 0.f, he = 0.f, cI = 0.f, cA = 0.f, cE = 0.f;
  if (giou) {
    we = __fadd_rn(__fadd_rn(fmaxf(d[0], t[0]), fmaxf(d[2], t[2])), 1.f);
    he = __fadd_rn(__fadd_rn(fmaxf(d[1], t[1]), fmaxf(d[3], t[3])), 1.f);
    const float E = __fmul_rn(we, he);
    R.loss_box = __fsub_rn(1.f, __fsub_rn(iou, __fdiv_rn(__fsub_rn(E, U), E)));
    if (NEED_GRAD) {
      const float invE = __fdiv_rn(1.f, E), U2 = __fmul_rn(U, U);
      cI = __fsub_rn(invE, __fdiv_rn(__fadd_rn(U, I), U2));
      cA = __fsub_rn(__fdiv_rn(I, U2), invE);
      cE = __fdiv_rn(U, __fmul_rn(E, E));
    }
  } else {
    R.loss_box = -logf(fmaxf(iou, eps));
    if (NEED_GRAD && iou >= eps) {
      cI = -__fdiv_rn(__fadd_rn(U, I), __fmul_rn(I, U));
      cA = __fdiv_rn(1.f, U);
    }
  }
  if (NEED_GRAD) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool horiz = (j & 1) == 0;             // l, r change the widths: their derivative carries the heights
      const float oA = horiz ? hp : wp, oI = horiz ? hi : wi, oE = horiz ? he : we;
      const float mI = d[j] <= t[j] ? __fmul_rn(cI, oI) : 0.f;
      const float mE = (giou && d[j] >= t[j]) ? __fmul_rn(cE, oE) : 0.f;
      const float dd = __fadd_rn(__fadd_rn(__fmul_rn(cA, oA), mI), mE);
      R.e[j] = __fmul_rn(R.c, __fmul_rn(dd, d[j]));
    }
  }
  return R;
}

template <int DT, bool GRAD>
__global__ __launch_bounds__(LT) void fcos_loss_kernel(const FlArgs A, const float* __restrict__ g,
                                                       const float* __restrict__ norm,
                                                       const double* __restrict__ scale_sums,
                                                       float* __restrict__ dscales, double* __restrict__ partials) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ double red[LWAVES][FPART];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float s_cls = 0.f, s_box = 0.f, s_ctr = 0.f;
  if (GRAD) {
    s_cls = __fdiv_rn(g[0], norm[0]);
    s_box = norm[1] > 0.f ? __fdiv_rn(g[1], norm[1]) : 0.f;
    s_ctr = __fdiv_rn(g[2], norm[2]);
    if (blockIdx.x == 0 && tid < A.L && A.has_scales) dscales[tid] = (float)((double)s_box * scale_sums[tid]);
  }
  double acc_cls = 0.0, acc_box = 0.0, acc_c = 0.0, acc_ctr = 0.0, acc_n = 0.0;
  for (int64_t g0 = (int64_t)blockIdx.x * LT; g0 < A.nchunks; g0 += (int64_t)gridDim.x * LT) {
    const int64_t gc = g0 + tid;
    for (int s = 0; s < A.L; ++s) {                          // s is uniform: the segment comes through scalar loads
      const FlSeg& S = A.seg[s];
      if (S.chunk0 + S.nchunks <= g0 || S.chunk0 >= g0 + LT) continue;
      if (gc >= S.chunk0 && gc < S.chunk0 + S.nchunks)
        acc_cls += fl_cls_chunk<DT, GRAD>(S, A, (uint32_t)(gc - S.chunk0), s_cls);
    }
  }
  for (int l = 0; l < A.L; ++l) {                            // uniform
    const FlLevel& V = A.lv[l];
    const int HW = V.HW, total = A.B * HW, off = A.seg[l].off;
    const float sc = A.has_scales ? A.scales[l] : 1.f;
    double acc_s = 0.0;
    for (int q0 = blockIdx.x * LT; q0 < total; q0 += gridDim.x * LT) {
      const int q = q0 + tid;
      if (q >= total) continue;
      const int b = q / HW, p = q - b * HW;
      const int64_t pt = (int64_t)b * A.N + off + p;
      const bool positive = A.labels[pt] > 0;
      float dr[4] = {0.f, 0.f, 0.f, 0.f}, dz = 0.f;
      if (positive) {
        float x[4], t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          x[j] = E::ld(((const T*)V.reg)[V.reg_nhwc ? ((int64_t)q * 4 + j) : (((int64_t)b * 4 + j) * HW + p)]);
        const f32x4_t tv = *(const f32x4_t*)(A.bt + pt * 4);
        t[0] = tv[0]; t[1] = tv[1]; t[2] = tv[2]; t[3] = tv[3];
        const float z = E::ld(((const T*)V.ctr)[q]);
        if (GRAD) {
          const FlPos R = fl_positive<true>(x, t, sc, A.giou, A.eps);
#pragma unroll
          for (int j = 0; j < 4; ++j) dr[j] = __fmul_rn(__fmul_rn(R.e[j], sc), s_box);
          dz = __fmul_rn(__fsub_rn(sigmoid(z), R.c), s_ctr);
        } else {
          FlPos R;
          if (A.has_scales) {
            R = fl_positive<true>(x, t, sc, A.giou, A.eps);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc_s += (double)__fmul_rn(R.e[j], x[j]);
          } else {
            R = fl_positive<false>(x, t, sc, A.giou, A.eps);
          }
          acc_box += (double)__fmul_rn(R.c, R.loss_box);
          acc_c += (double)R.c;
          acc_ctr += (double)__fsub_rn(softplus(z), __fmul_rn(R.c, z));
          acc_n += 1.0;
        }
      }
      if (GRAD) {
        T* dreg = (T*)V.dreg;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dreg[V.reg_nhwc ? ((int64_t)q * 4 + j) : (((int64_t)b * 4 + j) * HW + p)] = E::st(dr[j]);
        ((T*)V.dctr)[q] = E::st(dz);
      }
    }
    if (!GRAD && A.has_scales) {
      acc_s = wave_sum(acc_s);
      if (lane == 0) red[wave][P_SCALE + l] = acc_s;
    }
  }
  if (GRAD) return;
  // lanes -> xor tree, waves -> wave 0 .. 15 in order; thread k adds slot k and stores it
  acc_cls = wave_sum(acc_cls);
  acc_box = wave_sum(acc_box);
  acc_c = wave_sum(acc_c);
  acc_ctr = wave_sum(acc_ctr);
  acc_n = wave_sum(acc_n);
  if (lane == 0) {
    red[wave][P_CLS] = acc_cls;
    red[wave][P_BOX] = acc_box;
    red[wave][P_CSUM] = acc_c;
    red[wave][P_CTR] = acc_ctr;
    red[wave][P_NPOS] = acc_n;
  }
  __syncthreads();
  if (tid < FPART) {
    const bool live = tid < P_MAIN || (A.has_scales && tid >= P_SCALE && tid < P_SCALE + A.L);
    double s = 0.0;
    if (live)
      for (int w = 0; w < LWAVES; ++w) s += red[w][tid];
    partials[(size_t)blockIdx.x * FPART + tid] = s;
  }
}

// last launch: the partials in index order, the divisors, one rounding each
__global__ __launch_bounds__(LMAX_BLOCKS) void fcos_loss_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                         int B, int L, float* __restrict__ losses,
                                                                         float* __restrict__ norm,
                                                                         double* __restrict__ scale_sums) {
  __shared__ double stage[LMAX_BLOCKS][FPART + 1];
  __shared__ double tot[FPART];
  const int t = threadIdx.x;
  if (t < nparts)
    for (int k = 0; k < FPART; ++k) stage[t][k] = partials[(size_t)t * FPART + k];
  __syncthreads();
  if (t < FPART) {
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += stage[i][t];
    tot[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    const long long npos = (long long)tot[P_NPOS];             // a count: exact in fp64
    const float d_cls = (float)(npos + B), d_ctr = (float)(npos < 1 ? 1ll : npos);
    const double csum = tot[P_CSUM];
    losses[0] = (float)(tot[P_CLS] / (double)d_cls);
    losses[1] = csum > 0.0 ? (float)(tot[P_BOX] / csum) : 0.f;
    losses[2] = (float)(tot[P_CTR] / (double)d_ctr);
    norm[0] = d_cls;
    norm[1] = (float)csum;
    norm[2] = d_ctr;
  }
  if (scale_sums && t < L) scale_sums[t] = tot[P_SCALE + t];
}

struct FlPlan {
  FlArgs A;
  int blocks;
};

int fl_plan(const char* who, const tdn_fcos_level* levels, int L, int B, const tdn_fcos_loss_config* cfg, bool grad,
            FlPlan* out) {
  FcGeo G;
  if (fc_geo(who, levels, L, false, &G) != 0) return -1;
  TDN_CHECK(cfg, "%s: NULL config", who);
  if (tdn_check_batch(who, B) != 0) return -1;
  const int C = cfg->num_classes;
  TDN_CHECK(cfg->dtype == TDN_F32 || cfg->dtype == TDN_BF16 || cfg->dtype == TDN_F16, "%s: dtype %d", who, cfg->dtype);
  TDN_CHECK(C >= 1 && C <= TDN_LOSS_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_LOSS_MAX_CLASSES);
  TDN_CHECK(cfg->giou == 0 || cfg->giou == 1, "%s: giou must be 0 or 1", who);
  TDN_CHECK(cfg->gamma >= 0.f && cfg->gamma - cfg->gamma == 0.f && cfg->alpha >= 0.f && cfg->alpha <= 1.f,
            "%s: focal loss needs finite gamma >= 0 and alpha in [0, 1]", who);
  TDN_CHECK(cfg->eps > 0.f && cfg->eps < 1.f, "%s: eps must be in (0, 1)", who);
  memset(out, 0, sizeof(*out));
  FlArgs& A = out->A;
  A.L = L;
  A.B = B;
  A.N = G.N;
  A.C = C;
  A.giou = cfg->giou;
  A.eps = cfg->eps;
  A.P.focal = 1;
  A.P.gamma = cfg->gamma;
  A.P.alpha = cfg->alpha;
  A.P.one_minus_alpha = 1.f - cfg->alpha;
  const int V = cfg->dtype == TDN_F32 ? 4 : 8;
  int64_t chunks = 0, items = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_fcos_level& v = levels[l];
    const int64_t HW = (int64_t)v.H * v.W, n = (int64_t)B * C * HW;
    TDN_CHECK(n < (1ll << 31) && (int64_t)B * 4 * HW < (1ll << 31), "%s: level %d holds 2^31 elements or more", who, l);
    TDN_CHECK((v.cls_nhwc | v.reg_nhwc | 1) == 1, "%s: level %d: layout flags must be 0 or 1", who, l);
    FlSeg& S = A.seg[l];
    S.x = v.cls;
    S.dx = v.dcls;
    S.n = (uint32_t)n;
    S.nchunks = (uint32_t)((n + V - 1) / V);
    S.chunk0 = chunks;
    S.HW = (int)HW;
    S.nhwc = v.cls_nhwc;
    S.off = G.off[l];
    S.vec = (((uintptr_t)v.cls | (uintptr_t)v.dcls) & 15) == 0;
    chunks += S.nchunks;
    FlLevel& W = A.lv[l];
    W.reg = v.reg;
    W.ctr = v.ctr;
    W.dreg = v.dreg;
    W.dctr = v.dctr;
    W.HW = (int)HW;
    W.reg_nhwc = v.reg_nhwc;
    if ((int64_t)B * HW > items) items = (int64_t)B * HW;
    if (grad) TDN_CHECK(v.dcls && v.dreg && v.dctr, "%s: level %d has a NULL gradient pointer", who, l);
  }
  A.nchunks = chunks;
  out->blocks = tdn_grid_1d(chunks > items ? chunks : items, LT, LMAX_BLOCKS);
  return 0;
}

int fl_pointers(const char* who, const tdn_fcos_level* levels, int L, const int64_t* labels, const float* bt) {
  TDN_CHECK(labels && bt, "%s: NULL targets", who);
  for (int l = 0; l < L; ++l)
    TDN_CHECK(levels[l].cls && levels[l].reg && levels[l].ctr, "%s: level %d has a NULL pointer", who, l);
  return 0;
}

#define FL_LAUNCH(GRAD, dtype, grid, st, ...)                                                                          \
  do {                                                                                                                 \
    if ((dtype) == TDN_F32) TDN_LAUNCH((fcos_loss_kernel<TDN_F32, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);         \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((fcos_loss_kernel<TDN_F16, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);    \
    else TDN_LAUNCH((fcos_loss_kernel<TDN_BF16, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);                           \
  } while (0)

// ---- detections ----------------------------------------------------------------------------------------------------------
// The architecture of dense_detect.hip with A = 1: a key launch over the levels that select, one workgroup per (image,
// level) for the radix threshold, the ordered compaction and the dense rows, tdn_multiclass_nms (tdn_fcos_detections_soft:
// tdn_multiclass_nms_soft), a gather.
constexpr int FD_SEG_MAX = TDN_NMS_SEG_MAX;
constexpr int KEY_THREADS = 256;
constexpr int KEY_TILE = 8192;                 // floats of LDS per workgroup of the key kernel (32 KB)
constexpr int KEY_INFLIGHT = 4;                // 16-byte loads a thread of the key kernel keeps in flight

struct FdLevel {
  const void* cls;
  const void* reg;
  const void* ctr;
  int H, W, s;
  int n, k;                                    // points, points kept
  int koff, poff, keyoff;                      // prefix sums of k, of n, of n rounded up to 4 (key words)
  int blk_end, nblk, ta;                       // key launch: end of the level's workgroups, per image, points in each
  int cls_nhwc, reg_nhwc;
};
struct FdArgs {
  int L, B, C, K, N, NK;                       // K = sum k, N = sum n, NK = key words per image
  float scale;
  const int32_t* img_shapes;
  const float* scale_factors;
  const float* scales;
  FdLevel lv[TDN_FCOS_MAX_LEVELS];
};

__device__ __forceinline__ float fd_sigmoid(float v) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-v))); }

template <int DT>
__global__ __launch_bounds__(KEY_THREADS) void fcos_key_kernel(const FdArgs P, uint32_t* __restrict__ keys) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int VEC = E::V;
  __shared__ __attribute__((aligned(16))) float tile[KEY_TILE];
  const int tid = threadIdx.x, blk = blockIdx.x;
  int l = 0;
  while (l + 1 < P.L && blk >= P.lv[l].blk_end) ++l;
  const FdLevel& V = P.lv[l];
  const int r = blk - (V.blk_end - P.B * V.nblk);
  const int b = r / V.nblk, a0 = (r - b * V.nblk) * V.ta;
  const int na = min(V.ta, V.n - a0), C = P.C;
  uint32_t* out = keys + (int64_t)b * P.NK + V.keyoff;
  const T* ctr = (const T*)V.ctr + (int64_t)b * V.n;
  if (V.cls_nhwc) {
    // point i's classes are elements [i*C, (i+1)*C) of the image's block: the tile is ne contiguous elements, widened into
    // rows of odd pitch, so that the per-point reads below touch 32 different banks
    const int Cp = C | 1;
    const int ne = na * C;
    const T* src = (const T*)V.cls + ((int64_t)b * V.n + a0) * C;
    int done = 0;
    if (((uintptr_t)src & 15) == 0) {
      const int nv = ne / VEC;
      for (int v0 = tid; v0 < nv; v0 += KEY_THREADS * KEY_INFLIGHT) {
        Vec<T, VEC> raw[KEY_INFLIGHT];
#pragma unroll
        for (int u = 0; u < KEY_INFLIGHT; ++u) {
          const int v = v0 + u * KEY_THREADS;
          if (v < nv) raw[u] = *(const Vec<T, VEC>*)(src + (int64_t)v * VEC);
        }
#pragma unroll
        for (int u = 0; u < KEY_INFLIGHT; ++u) {
          const int v = v0 + u * KEY_THREADS;
          if (v < nv) {
            int a = (v * VEC) / C, c = v * VEC - a * C;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              tile[a * Cp + c] = E::ld(raw[u].v[j]);
              if (++c == C) {
                c = 0;
                ++a;
              }
            }
          }
        }
      }
      done = nv * VEC;
    }
    for (int e = done + tid; e < ne; e += KEY_THREADS) {
      const int a = e / C;
      tile[a * Cp + (e - a * C)] = E::ld(src[e]);
    }
    __syncthreads();
    if (tid < na) {
      const float* row = tile + tid * Cp;
      float m = row[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
      out[a0 + tid] = order_key(__fmul_rn(fd_sigmoid(m), fd_sigmoid(E::ld(ctr[a0 + tid]))));
    }
    return;
  }
  // NCHW: the lanes of a wavefront walk the pixels of one channel
  const int t = a0 + tid;
  if (t >= V.n) return;
  const T* src = (const T*)V.cls + (int64_t)b * C * V.n + t;
  float m = E::ld(src[0]);
  for (int c = 1; c < C; ++c) m = fmaxf(m, E::ld(src[(int64_t)c * V.n]));
  out[t] = order_key(__fmul_rn(fd_sigmoid(m), fd_sigmoid(E::ld(ctr[t]))));
}

// keys of one (image, level): contiguous words from a 16-byte boundary
struct FdKeyFetch {
  const uint32_t* k;
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
    if (cnt == TK_PER) {
      const uint4 lo = *(const uint4*)(k + i0), hi = *(const uint4*)(k + i0 + 4);
      kk[0] = lo.x; kk[1] = lo.y; kk[2] = lo.z; kk[3] = lo.w;
      kk[4] = hi.x; kk[5] = hi.y; kk[6] = hi.z; kk[7] = hi.w;
    } else {
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) kk[e] = k[i0 + e];
    }
  }
};

template <int DT>
__global__ __launch_bounds__(BLK) void fcos_select_decode_kernel(const FdArgs P, const uint32_t* __restrict__ keys,
                                                                 float* __restrict__ scores, float* __restrict__ boxes,
                                                                 int32_t* __restrict__ bidx, int64_t* __restrict__ pidx) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ int hist[TK_BINS];
  __shared__ int misc[TK_MISC];
  __shared__ int sel[FD_SEG_MAX];              // the kept points of a level that selects, ascending
  const int tid = threadIdx.x;
  const int s = blockIdx.x, b = s / P.L, l = s - b * P.L;
  const FdLevel& V = P.lv[l];
  const int n = V.n, k = V.k, C = P.C, W = V.W;
  const bool selecting = n > k;
  if (selecting) {
    const FdKeyFetch F{keys + (int64_t)b * P.NK + V.keyoff};
    int need;
    const uint32_t T0 = block_radix_threshold(F, n, k, hist, misc, &need);
    // keys > T0 and the first `need` keys == T0, in point order: a thread takes TK_PER consecutive points, so one scan of
    // both counts (packed: a step holds at most 8192 of either) places a whole step
    int gt_done = 0, ties_done = 0;
    for (int base = 0; base < n; base += TK_STEP) {
      const int i0 = base + tid * TK_PER;
      const int cnt = max(0, min(TK_PER, n - i0));
      uint32_t kk[TK_PER];
      if (cnt > 0) F(i0, cnt, kk);
      int ng = 0, nt = 0;
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) {
          ng += kk[e] > T0 ? 1 : 0;
          nt += kk[e] == T0 ? 1 : 0;
        }
      int tot;
      const int ex = block_excl_scan(ng | (nt << 16), misc, &tot);
      int tb = ties_done + (ex >> 16);                            // ties before this thread's first point
      int pos = gt_done + (ex & 0xFFFF) + min(tb, need);          // kept points before it
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) {
          if (kk[e] > T0) {
            sel[pos++] = i0 + e;
          } else if (kk[e] == T0) {
            if (tb < need) sel[pos++] = i0 + e;
            ++tb;
          }
        }
      gt_done += tot & 0xFFFF;
      ties_done += tot >> 16;
    }
    __syncthreads();
  }
  const int64_t row0 = (int64_t)b * P.K + V.koff;
  const int ih = P.img_shapes[2 * b], iw = P.img_shapes[2 * b + 1];
  const float xm = (float)(iw - 1), ym = (float)(ih - 1);
  const bool rescale = P.scale_factors || P.scale != 0.f;
  const float sf = P.scale_factors ? P.scale_factors[b] : P.scale;
  const float sc = P.scales ? P.scales[l] : 1.f;
  const T* reg = (const T*)V.reg + (int64_t)b * 4 * n;
  const T* cls = (const T*)V.cls + (int64_t)b * C * n;
  const T* ctr = (const T*)V.ctr + (int64_t)b * n;
  // one thread per kept row: the box, the background column, batch_idx, point_idx
  for (int r = tid; r < k; r += BLK) {
    const int i = selecting ? sel[r] : r;
    const int y = i / W, x = i - y * W;
    const float px = (float)(x * V.s + V.s / 2), py = (float)(y * V.s + V.s / 2);
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      d[j] = expf(__fmul_rn(sc, E::ld(reg[V.reg_nhwc ? ((int64_t)i * 4 + j) : ((int64_t)j * n + i)])));
    f32x4_t bx;
    bx[0] = fminf(fmaxf(__fsub_rn(px, d[0]), 0.f), xm);
    bx[1] = fminf(fmaxf(__fsub_rn(py, d[1]), 0.f), ym);
    bx[2] = fminf(fmaxf(__fadd_rn(px, d[2]), 0.f), xm);
    bx[3] = fminf(fmaxf(__fadd_rn(py, d[3]), 0.f), ym);
    if (rescale) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bx[e] = __fdiv_rn(bx[e], sf);
    }
    *(f32x4_t*)(boxes + (row0 + r) * 4) = bx;
    scores[(row0 + r) * (C + 1)] = 0.f;
    bidx[row0 + r] = b;
    pidx[row0 + r] = (int64_t)V.poff + i;
  }
  // one thread per (kept row, class), class fastest: the rows' stores are contiguous, and so are channels_last loads
  const int64_t total = (int64_t)k * C;
  for (int64_t q = tid; q < total; q += BLK) {
    const int r = (int)(q / C), c = (int)(q - (int64_t)r * C);
    const int i = selecting ? sel[r] : r;
    const float v = E::ld(cls[V.cls_nhwc ? ((int64_t)i * C + c) : ((int64_t)c * n + i)]);
    scores[(row0 + r) * (C + 1) + 1 + c] = __fmul_rn(fd_sigmoid(v), fd_sigmoid(E::ld(ctr[i])));
  }
}

__global__ void fcos_point_gather_kernel(const int64_t* __restrict__ row_idx, const int64_t* __restrict__ dense_pidx,
                                         int n, int64_t* __restrict__ point_idx) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) {
    const int64_t r = row_idx[q];
    point_idx[q] = r >= 0 ? dense_pidx[r] : -1;
  }
}

struct FdPlan {
  FdArgs A;
  int key_blocks, selecting;
  int64_t rows;                                // B * K
  int64_t nms_bytes;
};

// the checks and the geometry the plan query, the workspace query and the call share; pointers may be null
int fd_plan(const char* who, const tdn_fcos_level* levels, int L, int B, const tdn_fcos_det_config* cfg, FdPlan* out, bool soft = false) {
  FcGeo G;
  if (fc_geo(who, levels, L, false, &G) != 0) return -1;
  TDN_CHECK(cfg, "%s: NULL config", who);
  if (tdn_check_batch(who, B) != 0) return -1;
  const int C = cfg->num_classes;
  TDN_CHECK(cfg->dtype == TDN_F32 || cfg->dtype == TDN_BF16 || cfg->dtype == TDN_F16, "%s: dtype %d", who, cfg->dtype);
  TDN_CHECK(C >= 1 && C <= TDN_DET_MAX_CLASSES - 1, "%s: C=%d out of 1..%d", who, C, TDN_DET_MAX_CLASSES - 1);
  TDN_CHECK(cfg->nms_pre >= 0 && cfg->nms_pre <= FD_SEG_MAX, "%s: nms_pre=%d out of 0..%d", who, cfg->nms_pre,
            FD_SEG_MAX);
  TDN_CHECK(cfg->max_num >= 1 && cfg->max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, cfg->max_num,
            TDN_RPN_MAX_NUM);
  TDN_CHECK(cfg->score_thr - cfg->score_thr == 0.f && (soft || cfg->nms_thr - cfg->nms_thr == 0.f),
            "%s: score_thr / nms_thr must be finite", who);
  memset(out, 0, sizeof(*out));
  FdArgs& P = out->A;
  P.L = L;
  P.B = B;
  P.C = C;
  const int Cp = C | 1;
  int64_t K = 0, NK = 0, blocks = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_fcos_level& v = levels[l];
    FdLevel& V = P.lv[l];
    const int64_t n = (int64_t)v.H * v.W;
    TDN_CHECK((int64_t)B * (C > 4 ? C : 4) * n < (1ll << 31), "%s: level %d holds 2^31 elements or more", who, l);
    TDN_CHECK((v.cls_nhwc | v.reg_nhwc | 1) == 1, "%s: level %d: layout flags must be 0 or 1", who, l);
    V.cls = v.cls;
    V.reg = v.reg;
    V.ctr = v.ctr;
    V.H = v.H;
    V.W = v.W;
    V.s = v.stride;
    V.n = (int)n;
    V.k = (cfg->nms_pre > 0 && n > cfg->nms_pre) ? cfg->nms_pre : (int)n;
    TDN_CHECK(K + V.k <= TDN_DET_MAX_ROWS, "%s: more than %d dense rows", who, TDN_DET_MAX_ROWS);
    V.koff = (int)K;
    V.poff = G.off[l];
    V.keyoff = (int)NK;
    V.cls_nhwc = v.cls_nhwc;
    V.reg_nhwc = v.reg_nhwc;
    V.ta = V.cls_nhwc ? (KEY_TILE / Cp < KEY_THREADS ? KEY_TILE / Cp : KEY_THREADS) : KEY_THREADS;
    V.nblk = V.n > V.k ? (V.n + V.ta - 1) / V.ta : 0;
    blocks += (int64_t)B * V.nblk;
    TDN_CHECK(blocks < (1ll << 31), "%s: too many workgroups", who);
    V.blk_end = (int)blocks;
    out->selecting += V.n > V.k;
    K += V.k;
    NK += (n + 3) & ~3ll;
  }
  out->rows = (int64_t)B * K;
  TDN_CHECK(out->rows <= TDN_DET_MAX_ROWS, "%s: B * K = %lld dense rows (max %d)", who, (long long)out->rows,
            TDN_DET_MAX_ROWS);
  const int64_t seg = (int64_t)B * C * (out->rows < FD_SEG_MAX ? out->rows : FD_SEG_MAX);
  TDN_CHECK(seg < (1ll << 31), "%s: B * C * min(B * K, %d) segment rows do not fit 31 bits", who, FD_SEG_MAX);
  P.K = (int)K;
  P.N = G.N;
  P.NK = (int)NK;
  out->key_blocks = (int)blocks;
  out->nms_bytes = soft ? tdn_multiclass_nms_soft_workspace_bytes((int)out->rows, C + 1, B)
                        : tdn_multiclass_nms_workspace_bytes((int)out->rows, C + 1, B);
  return out->nms_bytes < 0 ? -1 : 0;
}

struct FdWs { uint32_t* keys; char* nms; int64_t bytes; };
FdWs fd_layout(const FdPlan& p, void* base) {   // a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<uint32_t>(p.selecting ? (int64_t)p.A.B * p.A.NK : 0), c.take<char>(p.nms_bytes), c.off};
}

#define FD_LAUNCH(kernel, dtype, grid, block, st, ...)                                              \
  do {                                                                                              \
    if ((dtype) == TDN_F32) TDN_LAUNCH(kernel<TDN_F32>, grid, block, 0, st, __VA_ARGS__);           \
    else if ((dtype) == TDN_F16) TDN_LAUNCH(kernel<TDN_F16>, grid, block, 0, st, __VA_ARGS__);      \
    else TDN_LAUNCH(kernel<TDN_BF16>, grid, block, 0, st, __VA_ARGS__);                             \
  } while (0)

}  // namespace

extern "C" int tdn_fcos_detections_plan(const tdn_fcos_level* levels, int nlevels, int B,
                                        const tdn_fcos_det_config* cfg, int32_t* out16) {
  FdPlan p;
  if (fd_plan("tdn_fcos_detections_plan", levels, nlevels, B, cfg, &p) != 0) return -1;
  TDN_CHECK(out16, "tdn_fcos_detections_plan: NULL output");
  memset(out16, 0, 16 * sizeof(int32_t));
  out16[0] = p.A.K;
  out16[1] = (int32_t)p.rows;
  out16[2] = p.A.N;
  out16[3] = p.selecting ? 7 : 6;
  out16[4] = p.key_blocks;
  out16[5] = p.selecting;
  const int64_t key_words = p.selecting ? (int64_t)p.A.B * p.A.NK : 0;
  out16[6] = key_words > INT32_MAX ? INT32_MAX : (int32_t)key_words;
  for (int l = 0; l < nlevels; ++l) out16[8 + l] = p.A.lv[l].k;
  return 0;
}

extern "C" int64_t tdn_fcos_detections_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B,
                                                       const tdn_fcos_det_config* cfg) {
  FdPlan p;
  if (fd_plan("tdn_fcos_detections", levels, nlevels, B, cfg, &p) != 0) return -1;
  return fd_layout(p, nullptr).bytes;
}

extern "C" int64_t tdn_fcos_detections_soft_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B,
                                                            const tdn_fcos_det_config* cfg) {
  FdPlan p;
  if (fd_plan("tdn_fcos_detections_soft", levels, nlevels, B, cfg, &p, true) != 0) return -1;
  return fd_layout(p, nullptr).bytes;
}

namespace {
// tdn_fcos_detections (soft == null) and tdn_fcos_detections_soft
int fd_run(const char* who, const tdn_fcos_level* levels, int nlevels, int B, const int32_t* img_shapes,
           const float* scale_factors, const float* scales, const tdn_fcos_det_config* cfg,
           const tdn_soft_nms_config* soft, float* dense_scores, float* dense_boxes, int32_t* batch_idx,
           int64_t* dense_point_idx, float* dets, int64_t* labels, int64_t* row_idx, int64_t* point_idx,
           int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  FdPlan p;
  if (fd_plan(who, levels, nlevels, B, cfg, &p, soft != nullptr) != 0) return -1;
  TDN_CHECK(scale_factors || cfg->scale_factor == 0.f ||
                (cfg->scale_factor > 0.f && cfg->scale_factor - cfg->scale_factor == 0.f),
            "%s: scale_factor must be positive and finite (0: none)", who);
  TDN_CHECK(img_shapes && dense_scores && dense_boxes && batch_idx && dense_point_idx && dets && labels && row_idx &&
                point_idx && counts, "%s: NULL pointer", who);
  for (int l = 0; l < nlevels; ++l)
    TDN_CHECK(levels[l].cls && levels[l].reg && levels[l].ctr, "%s: level %d has a NULL pointer", who, l);
  const FdWs w = fd_layout(p, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  FdArgs& P = p.A;
  P.img_shapes = img_shapes;
  P.scale_factors = scale_factors;
  P.scale = scale_factors ? 0.f : cfg->scale_factor;
  P.scales = scales;
  hipStream_t st = (hipStream_t)stream;
  if (p.key_blocks > 0) {
    FD_LAUNCH(fcos_key_kernel, cfg->dtype, dim3(p.key_blocks), dim3(KEY_THREADS), st, P, w.keys);
    TDN_LAUNCH_CHECK();
  }
  FD_LAUNCH(fcos_select_decode_kernel, cfg->dtype, dim3(B * nlevels), dim3(BLK), st, P, (const uint32_t*)w.keys,
            dense_scores, dense_boxes, batch_idx, dense_point_idx);
  TDN_LAUNCH_CHECK();
  const int rc = soft ? tdn_multiclass_nms_soft(dense_boxes, 4, dense_scores, batch_idx, 4, (int)p.rows, P.C + 1, B,
                                                cfg->score_thr, soft, cfg->max_num, dets, labels, row_idx, counts, w.nms,
                                                p.nms_bytes, stream)
                      : tdn_multiclass_nms(dense_boxes, 4, dense_scores, batch_idx, 4, (int)p.rows, P.C + 1, B,
                                           cfg->score_thr, cfg->nms_thr, cfg->max_num, dets, labels, row_idx, counts,
                                           w.nms, p.nms_bytes, stream);
  if (rc != 0) return rc;
  const int nd = B * cfg->max_num;
  TDN_LAUNCH(fcos_point_gather_kernel, dim3((nd + 255) / 256), dim3(256), 0, st, (const int64_t*)row_idx,
             (const int64_t*)dense_point_idx, nd, point_idx);
  TDN_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int tdn_fcos_detections(const tdn_fcos_level* levels, int nlevels, int B, const int32_t* img_shapes,
                                   const float* scale_factors, const float* scales, const tdn_fcos_det_config* cfg,
                                   float* dense_scores, float* dense_boxes, int32_t* batch_idx,
                                   int64_t* dense_point_idx, float* dets, int64_t* labels, int64_t* row_idx,
                                   int64_t* point_idx, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  return fd_run("tdn_fcos_detections", levels, nlevels, B, img_shapes, scale_factors, scales, cfg, nullptr, dense_scores,
                dense_boxes, batch_idx, dense_point_idx, dets, labels, row_idx, point_idx, counts, workspace,
                workspace_bytes, stream);
}

extern "C" int tdn_fcos_detections_soft(const tdn_fcos_level* levels, int nlevels, int B, const int32_t* img_shapes,
                                        const float* scale_factors, const float* scales,
                                        const tdn_fcos_det_config* cfg, const tdn_soft_nms_config* soft,
                                        float* dense_scores, float* dense_boxes, int32_t* batch_idx,
                                        int64_t* dense_point_idx, float* dets, int64_t* labels, int64_t* row_idx,
                                        int64_t* point_idx, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  const char* who = "tdn_fcos_detections_soft";
  if (tdn_soft_nms_check(who, soft) != 0) return -1;  // before the first launch
  return fd_run(who, levels, nlevels, B, img_shapes, scale_factors, scales, cfg, soft, dense_scores, dense_boxes,
                batch_idx, dense_point_idx, dets, labels, row_idx, point_idx, counts, workspace, workspace_bytes, stream);
}

extern "C" int64_t tdn_fcos_loss_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B,
                                                 const tdn_fcos_loss_config* cfg) {
  FlPlan p;
  if (fl_plan("tdn_fcos_loss_workspace_bytes", levels, nlevels, B, cfg, false, &p) != 0) return -1;
  return align256((int64_t)p.blocks * FPART * (int64_t)sizeof(double));
}

extern "C" int tdn_fcos_loss_fwd(const tdn_fcos_level* levels, int nlevels, int B, const tdn_fcos_loss_config* cfg,
                                 const int64_t* labels, const float* bbox_targets, const float* scales, float* losses,
                                 float* norm, double* scale_sums, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  const char* who = "tdn_fcos_loss_fwd";
  FlPlan p;
  if (fl_plan(who, levels, nlevels, B, cfg, false, &p) != 0) return -1;
  if (fl_pointers(who, levels, nlevels, labels, bbox_targets) != 0) return -1;
  TDN_CHECK(losses && norm, "%s: NULL output", who);
  TDN_CHECK((scales != nullptr) == (scale_sums != nullptr), "%s: scale_sums goes with scales", who);
  if (tdn_check_ws(who, workspace, workspace_bytes, align256((int64_t)p.blocks * FPART * (int64_t)sizeof(double))) != 0)
    return -1;
  p.A.labels = labels;
  p.A.bt = bbox_targets;
  p.A.scales = scales;
  p.A.has_scales = scales ? 1 : 0;
  double* partials = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  FL_LAUNCH(false, cfg->dtype, dim3(p.blocks), st, p.A, (const float*)nullptr, (const float*)nullptr,
            (const double*)nullptr, (float*)nullptr, partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(fcos_loss_finalize_kernel, dim3(1), dim3(LMAX_BLOCKS), 0, st, (const double*)partials, p.blocks, B, nlevels,
             losses, norm, scale_sums);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_fcos_loss_bwd(const tdn_fcos_level* levels, int nlevels, int B, const tdn_fcos_loss_config* cfg,
                                 const int64_t* labels, const float* bbox_targets, const float* scales, const float* g,
                                 const float* norm, const double* scale_sums, float* dscales, void* stream) {
  const char* who = "tdn_fcos_loss_bwd";
  FlPlan p;
  if (fl_plan(who, levels, nlevels, B, cfg, true, &p) != 0) return -1;
  if (fl_pointers(who, levels, nlevels, labels, bbox_targets) != 0) return -1;
  TDN_CHECK(g && norm, "%s: NULL cotangent / divisors", who);
  TDN_CHECK((scales != nullptr) == (scale_sums != nullptr) && (scales != nullptr) == (dscales != nullptr),
            "%s: scale_sums and dscales go with scales", who);
  p.A.labels = labels;
  p.A.bt = bbox_targets;
  p.A.scales = scales;
  p.A.has_scales = scales ? 1 : 0;
  FL_LAUNCH(true, cfg->dtype, dim3(p.blocks), (hipStream_t)stream, p.A, g, norm, scale_sums, dscales,
            (double*)nullptr);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_fcos_points(const tdn_fcos_level* levels, int nlevels, float* points, void* stream) {
  const char* who = "tdn_fcos_points";
  FcGeo G;
  if (fc_geo(who, levels, nlevels, false, &G) != 0) return -1;
  TDN_CHECK(points, "%s: NULL output", who);
  TDN_LAUNCH(fcos_points_kernel, dim3((G.N + FT - 1) / FT), dim3(FT), 0, (hipStream_t)stream, G, points);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_fcos_target_workspace_bytes(const tdn_fcos_level* levels, int nlevels, int B, int G) {
  FcGeo Geo;
  if (fc_target_plan("tdn_fcos_target_workspace_bytes", levels, nlevels, B, G, &Geo) != 0) return -1;
  return align256((int64_t)B * ((Geo.N + FT - 1) / FT) * (int64_t)sizeof(int32_t));
}

extern "C" int tdn_fcos_target(const tdn_fcos_level* levels, int nlevels, int B, const float* gt,
                               const int64_t* gt_labels, const int32_t* gt_counts, int G, float radius,
                               int64_t* labels, float* bbox_targets, int32_t* assigned, int32_t* num_pos,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_fcos_target";
  FcGeo Geo;
  if (fc_target_plan(who, levels, nlevels, B, G, &Geo) != 0) return -1;
  TDN_CHECK(radius >= 0.f && radius - radius == 0.f, "%s: radius must be finite and >= 0 (0: no centre sampling)", who);
  TDN_CHECK(G == 0 || (gt && gt_counts), "%s: NULL ground truths", who);
  TDN_CHECK(labels && bbox_targets && assigned && num_pos, "%s: NULL output", who);
  const int nblk = (Geo.N + FT - 1) / FT;
  if (tdn_check_ws(who, workspace, workspace_bytes, align256((int64_t)B * nblk * (int64_t)sizeof(int32_t))) != 0)
    return -1;
  int32_t* part = (int32_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  TDN_LAUNCH(fcos_target_kernel, dim3(nblk, B), dim3(FT), 0, st, Geo, gt, G > 0 ? gt_labels : (const int64_t*)nullptr,
             gt_counts, G, radius, labels, bbox_targets, assigned, part);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(fcos_count_kernel, dim3(B), dim3(FT), 0, st, (const int32_t*)part, nblk, num_pos);
  TDN_LAUNCH_CHECK();
  return 0;
}
