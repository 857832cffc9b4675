// Guided Anchoring (DESIGN.md §4w has the spec, tests/ga_ref.py restates it): location targets, shape targets by
// approx-max-IoU assignment, the location + shape loss with its gradients, the guided anchors with their mask, and RPN
// proposals from them.
//
// Semantics are the project's own spec in the mmdetection-v1 lineage (GuidedAnchorHead: ga_loc_target, ga_shape_target
// with ApproxMaxIoUAssigner, loss_loc / loss_shape, get_anchors) on '+1' boxes, strict IEEE fp32 in the spec's operation
// order (this file is compiled with -ffp-contract=off).  Locations are level-major, (y*W + x) within a level.
// No memset, no atomics on floats, no inter-workgroup waits, no allocation; sums are fp64 in an order fixed by the
// shapes and the only atomics are integer maxima / minima, so every output is a pure function of the inputs.
#include "nms_core.h"
#include "select_core.h"
#include "delta_core.h"
#include "loss_core.h"
#include "target_host.h"
#include "proposal_host.h"
#include <limits.h>
#include <math.h>
#include <string.h>

namespace {

constexpr int MAXG = TDN_TARGET_MAX_GT;
constexpr int MAXL = TDN_LOSS_MAX_LEVELS;

// ---- the pyramid ---------------------------------------------------------------------------------------------------------
struct GaGeo {
  int L, N;
  int off[MAXL + 1];               // prefix sums of H*W
  int H[MAXL], W[MAXL], s[MAXL];
};

// location i of the pyramid: its level and through *h / *w its cell
__device__ __forceinline__ int ga_locate(const GaGeo& G, int i, int* h, int* w) {
  int l = 0;
  while (l + 1 < G.L && i >= G.off[l + 1]) ++l;
  const int p = i - G.off[l], W = G.W[l];
  *h = p / W;
  *w = p - *h * W;
  return l;
}

int ga_geo(const char* who, const tdn_ga_level* levels, int L, bool strides, GaGeo* out) {
  TDN_CHECK(levels, "%s: NULL levels", who);
  TDN_CHECK(L >= 1 && L <= MAXL, "%s: %d levels (1..%d)", who, L, MAXL);
  memset(out, 0, sizeof(*out));
  out->L = L;
  int64_t N = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_ga_level& v = levels[l];
    TDN_CHECK(v.H >= 1 && v.W >= 1, "%s: level %d is %d x %d", who, l, v.H, v.W);
    if (strides) {
      TDN_CHECK(v.stride >= 1 && v.stride <= (1 << 15), "%s: level %d has stride %d (1..32768)", who, l, v.stride);
      TDN_CHECK((int64_t)v.H * v.stride < (1 << 24) && (int64_t)v.W * v.stride < (1 << 24),
                "%s: level %d spans 2^24 pixels or more", who, l);
    }
    out->off[l] = (int)N;
    out->H[l] = v.H;
    out->W[l] = v.W;
    out->s[l] = v.stride;
    N += (int64_t)v.H * v.W;
    TDN_CHECK(N <= TDN_TARGET_MAX_BOXES, "%s: more than %d locations per image", who, TDN_TARGET_MAX_BOXES);
  }
  for (int l = L; l <= MAXL; ++l) out->off[l] = (int)N;
  out->N = (int)N;
  return 0;
}

int ga_check_gt(const char* who, int B, int G) {
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(G >= 0 && G <= MAXG, "%s: G=%d ground truths per image (max %d)", who, G, MAXG);
  return 0;
}

__device__ __forceinline__ int gt_count(const int32_t* gt_counts, int b, int G) {
  return G > 0 ? min(max(gt_counts[b], 0), G) : 0;
}

// ---- location targets ------------------------------------------------------------------------------------------------------
// One thread per (image, location), the image's ground truths and their levels in LDS, walked in ascending j: a later
// box's ignore region erases an earlier box's weight 1 but not its target 1, as the overwrites of the slice assignments
// it restates do.
constexpr int GT_ = 256;

struct GlArgs {
  GaGeo G;
  float thr[MAXL];                 // thr[k - 1] = t_k
  float rc, cc, ri, ci;            // (ratio', 1 - ratio') of the centre and of the ignore region
  int NG;
};

// is cell (x, y) inside calc_region(g, ratio') clamped to the map?  Everything is an integer held in fp32.
__device__ __forceinline__ bool ga_in_region(const f32x4_t g, float r, float c, float xm, float ym, float x, float y) {
  const float x1 = rintf(__fadd_rn(__fmul_rn(c, g[0]), __fmul_rn(r, g[2])));
  const float y1 = rintf(__fadd_rn(__fmul_rn(c, g[1]), __fmul_rn(r, g[3])));
  const float x2 = rintf(__fadd_rn(__fmul_rn(r, g[0]), __fmul_rn(c, g[2])));
  const float y2 = rintf(__fadd_rn(__fmul_rn(r, g[1]), __fmul_rn(c, g[3])));
  return x >= fminf(fmaxf(x1, 0.f), xm) && x <= fminf(fmaxf(x2, 0.f), xm) && y >= fminf(fmaxf(y1, 0.f), ym) &&
         y <= fminf(fmaxf(y2, 0.f), ym);
}

__global__ __launch_bounds__(GT_) void ga_loc_target_kernel(const GlArgs A, const float* __restrict__ gt,
                                                            const int32_t* __restrict__ gt_counts,
                                                            int64_t* __restrict__ loc_targets,
                                                            float* __restrict__ loc_weights) {
  __shared__ f32x4_t sbox[MAXG];
  __shared__ int slvl[MAXG];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int cnt = gt_count(gt_counts, b, A.NG);
  for (int j = tid; j < cnt; j += GT_) {
    const f32x4_t bx = *(const f32x4_t*)(gt + ((int64_t)b * A.NG + j) * 4);
    const float area = box_area(bx);
    int lv = 0;
    for (int k = 1; k < A.G.L; ++k) lv += area >= A.thr[k - 1] ? 1 : 0;
    sbox[j] = bx;
    slvl[j] = lv;
  }
  __syncthreads();
  const int i = blockIdx.x * GT_ + tid;
  if (i >= A.G.N) return;
  int h, w;
  const int l = ga_locate(A.G, i, &h, &w);
  const float s = (float)A.G.s[l], x = (float)w, y = (float)h;
  const float xm = (float)(A.G.W[l] - 1), ym = (float)(A.G.H[l] - 1);
  int t = 0, ig = 0;
  float wgt = -1.f;
  for (int j = 0; j < cnt; ++j) {
    const int d = slvl[j] - l;
    if (d < -1 || d > 1) continue;
    const f32x4_t bx = sbox[j];
    const f32x4_t g = {__fdiv_rn(bx[0], s), __fdiv_rn(bx[1], s), __fdiv_rn(bx[2], s), __fdiv_rn(bx[3], s)};
    const bool in_ig = ga_in_region(g, A.ri, A.ci, xm, ym, x, y);
    if (d == 0) {
      if (in_ig) wgt = 0.f;
      if (ga_in_region(g, A.rc, A.cc, xm, ym, x, y)) {
        t = 1;
        wgt = 1.f;
      }
    } else if (in_ig) {
      ig = 1;
    }
  }
  if (wgt < 0.f) wgt = ig ? 0.f : 0.1f;
  const int64_t q = (int64_t)b * A.G.N + i;
  loc_targets[q] = t;
  loc_weights[q] = wgt;
}

// ---- shape targets: approx-max-IoU assignment ------------------------------------------------------------------------------
// tdn_anchor_target's launch structure (target.hip) with two new assign passes: a lane owns a location and holds its A
// approximating boxes in registers; the overlap with ground truth j is the maximum over them.  Both passes run the same
// instructions on the same values, so pass 2 meets pass 1's column maxima bit for bit.
constexpr int P1_THREADS = 256;
constexpr int P1_PER = 4;                      // locations per thread: 1024 per workgroup share one LDS copy of the gts

struct GsArgs {
  const float* approxs;            // [N][A][4]
  const uint8_t* valid;            // [N*A] (vstride 0) or [B][N*A], or NULL
  int64_t vstride;
  const int32_t* img_shapes;       // with border >= 0: [B][2] = (h, w)
  int border;
  const float* gt;                 // [B][G][4]
  const int32_t* gt_counts;
  int N, G, A, all;
  float pos_thr, neg_thr, min_pos;
};

// the location's boxes and their areas; true if it takes part: one of them is flagged valid and inside the image
template <int AMAX>
__device__ __forceinline__ bool ga_fetch(const GsArgs& S, int b, int i, f32x4_t* bx, float* area) {
  bool part = false;
  float lo = 0.f, hy = 0.f, hx = 0.f;
  if (S.border >= 0) {
    lo = (float)(-S.border);
    hy = (float)(S.img_shapes[2 * b] + S.border);
    hx = (float)(S.img_shapes[2 * b + 1] + S.border);
  }
#pragma unroll
  for (int a = 0; a < AMAX; ++a)
    if (a < S.A) {                             // uniform
      const int64_t r = (int64_t)i * S.A + a;
      const f32x4_t v = *(const f32x4_t*)(S.approxs + r * 4);
      bx[a] = v;
      area[a] = box_area(v);
      bool ok = !S.valid || S.valid[b * S.vstride + r] != 0;
      if (S.border >= 0) ok = ok && v[0] >= lo && v[1] >= lo && v[2] < hx && v[3] < hy;
      part = part || ok;
    }
  return part;
}

template <int AMAX>
__device__ __forceinline__ float ga_overlap(const GsArgs& S, const f32x4_t* bx, const float* area, const f32x4_t g,
                                            float garea) {
  float v = box_iou2(bx[0], area[0], g, garea);
#pragma unroll
  for (int a = 1; a < AMAX; ++a)
    if (a < S.A) {
      const float u = box_iou2(bx[a], area[a], g, garea);
      v = u > v ? u : v;
    }
  return v;
}

template <int AMAX>
__global__ __launch_bounds__(P1_THREADS) void ga_assign_pass1_kernel(const GsArgs S, int32_t* __restrict__ assigned,
                                                                     float* __restrict__ max_overlaps,
                                                                     uint32_t* colmax) {
  __shared__ f32x4_t sgt[MAXG];
  __shared__ float sarea[MAXG];
  __shared__ uint32_t scol[MAXG];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int Gb = gt_count(S.gt_counts, b, S.G);
  for (int j = tid; j < Gb; j += P1_THREADS) {
    const f32x4_t g = *(const f32x4_t*)(S.gt + ((int64_t)b * S.G + j) * 4);
    sgt[j] = g;
    sarea[j] = box_area(g);
    scol[j] = 0u;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < P1_PER; ++k) {
    const int i = (blockIdx.x * P1_PER + k) * P1_THREADS + tid;
    if (i >= S.N) break;
    f32x4_t bx[AMAX];
    float area[AMAX];
    const bool ok = ga_fetch<AMAX>(S, b, i, bx, area);
    int a = -1;
    float mx = 0.f;
    if (ok) {
      if (Gb == 0) {
        a = 0;
      } else {
        int am = 0;
        mx = -1.f;
        for (int j = 0; j < Gb; ++j) {
          const float v = ga_overlap<AMAX>(S, bx, area, sgt[j], sarea[j]);
          if (v > mx) {
            mx = v;
            am = j;
          }
          const uint32_t bits = __float_as_uint(v);
          if (v > 0.f && bits > scol[j]) atomicMax(&scol[j], bits);   // a stale read only costs a redundant atomic
        }
        if (mx >= 0.f && mx < S.neg_thr) a = 0;
        if (mx >= S.pos_thr) a = am + 1;
        if (!(mx >= 0.f)) mx = 0.f;
      }
    }
    assigned[(int64_t)b * S.N + i] = a;
    max_overlaps[(int64_t)b * S.N + i] = mx;
  }
  __syncthreads();
  for (int j = tid; j < Gb; j += P1_THREADS) {
    const uint32_t v = scol[j];
    uint32_t* g = colmax + b * S.G + j;
    if (v != 0u && v > *(volatile uint32_t*)g) atomicMax(g, v);     // a stale read only costs a redundant atomic
  }
}

template <int AMAX>
__global__ __launch_bounds__(P1_THREADS) void ga_assign_pass2_kernel(const GsArgs S, int32_t* __restrict__ assigned,
                                                                     const uint32_t* __restrict__ colmax, int* first) {
  __shared__ f32x4_t sgt[MAXG];
  __shared__ float sarea[MAXG];
  __shared__ float sgm[MAXG];                  // the column maximum, or -1 where it is below min_pos_iou
  __shared__ int sfirst[MAXG];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int Gb = gt_count(S.gt_counts, b, S.G);
  if (Gb == 0) return;
  for (int j = tid; j < Gb; j += P1_THREADS) {
    const f32x4_t g = *(const f32x4_t*)(S.gt + ((int64_t)b * S.G + j) * 4);
    sgt[j] = g;
    sarea[j] = box_area(g);
    const float gm = __uint_as_float(colmax[b * S.G + j]);
    sgm[j] = gm >= S.min_pos ? gm : -1.f;
    sfirst[j] = INT_MAX;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < P1_PER; ++k) {
    const int i = (blockIdx.x * P1_PER + k) * P1_THREADS + tid;
    if (i >= S.N) break;
    f32x4_t bx[AMAX];
    float area[AMAX];
    if (!ga_fetch<AMAX>(S, b, i, bx, area)) continue;
    int a = -1;
    for (int j = 0; j < Gb; ++j) {
      const float v = ga_overlap<AMAX>(S, bx, area, sgt[j], sarea[j]);
      if (v == sgm[j]) {
        a = j + 1;                             // the highest such j stays
        if (!S.all) atomicMin(&sfirst[j], i);
      }
    }
    if (S.all && a > 0) assigned[(int64_t)b * S.N + i] = a;
  }
  if (S.all) return;
  __syncthreads();
  for (int j = tid; j < Gb; j += P1_THREADS)
    if (sfirst[j] != INT_MAX) atomicMin(first + b * S.G + j, sfirst[j]);
}

// sampling off: every positive and every negative; one workgroup per image writes both masks and the two counts
__global__ __launch_bounds__(1024) void ga_take_all_kernel(const int32_t* __restrict__ assigned, int N,
                                                           uint8_t* __restrict__ pos_mask, uint8_t* __restrict__ neg_mask,
                                                           int32_t* __restrict__ num_pos, int32_t* __restrict__ num_neg) {
  __shared__ int cnt[2];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  int cp = 0, cn = 0;
  for (int i = tid; i < N; i += 1024) {
    const int a = assigned[(int64_t)b * N + i];
    pos_mask[(int64_t)b * N + i] = a > 0 ? 1 : 0;
    neg_mask[(int64_t)b * N + i] = a == 0 ? 1 : 0;
    cp += a > 0 ? 1 : 0;
    cn += a == 0 ? 1 : 0;
  }
  if (cp) atomicAdd(&cnt[0], cp);              // integer adds: any order gives the same sum
  if (cn) atomicAdd(&cnt[1], cn);
  __syncthreads();
  if (tid == 0) {
    num_pos[b] = cnt[0];
    num_neg[b] = cnt[1];
  }
}

__global__ __launch_bounds__(256) void ga_shape_fill_kernel(const float* __restrict__ squares,
                                                            const float* __restrict__ gt, int N, int G,
                                                            const int32_t* __restrict__ assigned,
                                                            const uint8_t* __restrict__ pos_mask,
                                                            float* __restrict__ bbox_anchors,
                                                            float* __restrict__ bbox_gts,
                                                            float* __restrict__ bbox_weights) {
  const int b = blockIdx.y;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
    const int64_t q = (int64_t)b * N + i;
    f32x4_t an = {0.f, 0.f, 0.f, 0.f}, g = an, w = an;
    if (pos_mask[q] != 0) {
      an = *(const f32x4_t*)(squares + (int64_t)i * 4);
      g = *(const f32x4_t*)(gt + ((int64_t)b * G + assigned[q] - 1) * 4);
      w = (f32x4_t){1.f, 1.f, 1.f, 1.f};
    }
    *(f32x4_t*)(bbox_anchors + q * 4) = an;
    *(f32x4_t*)(bbox_gts + q * 4) = g;
    *(f32x4_t*)(bbox_weights + q * 4) = w;
  }
}

// column maxima, first indices, the two masks
struct GsWs { int64_t words; uint32_t* colmax; int* first; uint8_t *pos_mask, *neg_mask; int64_t bytes; };
GsWs gs_layout(int B, int64_t N, int G, void* base) {   // a braced list is evaluated left to right
  const int64_t words = (int64_t)B * (G > 0 ? G : 1), n = (int64_t)B * (N > 0 ? N : 1);
  tdn_carver c{(char*)base, 0};
  return {words, c.take<uint32_t>(words), c.take<int>(words), c.take<uint8_t>(n), c.take<uint8_t>(n), c.off};
}

int gs_check_dims(const char* who, int B, int64_t N, int G, int A) {
  if (ga_check_gt(who, B, G) != 0) return -1;
  TDN_CHECK(A >= 1 && A <= TDN_GA_MAX_APPROX, "%s: A=%d approxs per location (1..%d)", who, A, TDN_GA_MAX_APPROX);
  TDN_CHECK(N >= 1 && N <= TDN_TARGET_MAX_BOXES, "%s: %lld locations per image (1..%d)", who, (long long)N,
            TDN_TARGET_MAX_BOXES);
  return 0;
}

#define GS_LAUNCH(kernel, A_, grid, st, ...)                                                            \
  do {                                                                                                  \
    if ((A_) <= 1) TDN_LAUNCH(kernel<1>, grid, dim3(P1_THREADS), 0, st, __VA_ARGS__);                   \
    else if ((A_) <= 3) TDN_LAUNCH(kernel<3>, grid, dim3(P1_THREADS), 0, st, __VA_ARGS__);              \
    else if ((A_) <= 9) TDN_LAUNCH(kernel<9>, grid, dim3(P1_THREADS), 0, st, __VA_ARGS__);              \
    else TDN_LAUNCH(kernel<TDN_GA_MAX_APPROX>, grid, dim3(P1_THREADS), 0, st, __VA_ARGS__);             \
  } while (0)

// ---- the head outputs --------------------------------------------------------------------------------------------------------
struct GhLevel {
  const void* loc;
  const void* shape;
  void* dloc;
  void* dshape;
  int32_t HW, off, shape_nhwc, pad;
};

// element k (0: dw, 1: dh) of location p of image b
__device__ __forceinline__ int64_t ga_shape_index(const GhLevel& V, int b, int p, int k) {
  return V.shape_nhwc ? (((int64_t)b * V.HW + p) * 2 + k) : (((int64_t)b * 2 + k) * V.HW + p);
}

// ---- guided anchors ----------------------------------------------------------------------------------------------------------
struct GdArgs {
  GhLevel lv[MAXL];
  GaGeo G;
  f32x4_t means, stds;
  float max_ratio, thr;
  int use_loc;
};

template <int DT>
__global__ __launch_bounds__(GT_) void guided_anchors_kernel(const GdArgs A, const float* __restrict__ squares,
                                                             float* __restrict__ anchors, uint8_t* __restrict__ mask) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const int b = blockIdx.y, i = blockIdx.x * GT_ + threadIdx.x;
  if (i >= A.G.N) return;
  int l = 0;
  while (l + 1 < A.G.L && i >= A.G.off[l + 1]) ++l;
  const GhLevel& V = A.lv[l];
  const int p = i - V.off;
  const float dw = E::ld(((const T*)V.shape)[ga_shape_index(V, b, p, 0)]);
  const float dh = E::ld(((const T*)V.shape)[ga_shape_index(V, b, p, 1)]);
  const f32x4_t sq = *(const f32x4_t*)(squares + (int64_t)i * 4);
  const int64_t q = (int64_t)b * A.G.N + i;
  *(f32x4_t*)(anchors + q * 4) = decode_box(sq, (f32x4_t){0.f, 0.f, dw, dh}, A.means, A.stds, A.max_ratio, -1, -1);
  uint8_t m = 1;
  if (A.use_loc) m = E::ld(((const T*)V.loc)[(int64_t)b * V.HW + p]) >= A.thr ? 1 : 0;
  mask[q] = m;
}

// ---- loss ----------------------------------------------------------------------------------------------------------------
// One kernel, two walks, as fcos.hip's: the location logits of every level as the flat arrays they are in memory, in
// chunks of 16 bytes (loss_core.h's segment walk, one channel); then, level by level, one thread per (image, location):
// a row with bbox_weights[..][0] > 0 reads its two shape outputs, its anchor and its ground truth, every other row reads
// that weight only.  GRAD: the same walks write every gradient element.
constexpr int LT = 1024;
constexpr int LWAVES = LT / 64;
constexpr int LMAX_BLOCKS = 256;
constexpr int GPART = 2;            // doubles per partial: the location sum, the shape sum

struct GlossArgs {
  HeadSeg seg[MAXL];                // the location logits
  GhLevel lv[MAXL];
  int32_t L, B, N, pad;
  int64_t nchunks;
  const int64_t* loc_targets;
  const float* loc_weights;
  const float* anchors;
  const float* gts;
  const float* bw;
  f32x4_t means, stds;
  float max_ratio, beta, half_beta, eps;
  ClsParams P;
};

template <int DT, bool GRAD>
__device__ __forceinline__ double ga_loc_chunk(const HeadSeg& S, const GlossArgs& A, uint32_t lc, float s_loc) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  const uint32_t m0 = lc * (uint32_t)V;
  const int cnt = (int)min((uint32_t)V, S.n - m0);
  const Vec<T, V> in = head_load<DT>(S, m0, cnt);
  Vec<T, V> out;
  uint32_t b = m0 / (uint32_t)S.HW, p = m0 - b * (uint32_t)S.HW;   // one channel: both layouts are (b, p)
  double sum = 0.0;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float res = 0.f;
    if (e < cnt) {
      const int64_t idx = (int64_t)b * A.N + S.off + p;
      const float w = A.loc_weights[idx];
      if (w != 0.f) {                              // a weight of exactly 0: the logit is never evaluated
        const float v = cls_elem<GRAD>(E::ld(in.v[e]), A.loc_targets[idx] == 1, A.P);
        if (GRAD) res = __fmul_rn(__fmul_rn(w, v), s_loc);
        else sum += (double)__fmul_rn(w, v);
      }
      if (++p == (uint32_t)S.HW) { p = 0; ++b; }
    }
    if (GRAD) out.v[e] = E::st(res);
  }
  if (GRAD) head_store<DT>(S, m0, cnt, out);
  return sum;
}

// smooth-L1 shaping of a bounded-IoU term l >= 0 with knee beta, or its derivative
template <bool GRAD>
__device__ __forceinline__ float ga_shape_knee(float l, float beta, float half_beta) {
  if (l < beta) return GRAD ? __fdiv_rn(l, beta) : __fdiv_rn(__fmul_rn(__fmul_rn(0.5f, l), l), beta);
  return GRAD ? 1.f : __fsub_rn(l, half_beta);
}

// One axis of bounded_iou_loss: (o0, o1) the side of the decoded box, (g0, g1) the ground truth's.  Returns the weighted
// loss of the centre term and of the size term.  GRAD: *grad = the derivative of that with respect to the raw shape
// output d instead (the centre of the decoded box does not depend on d); (a0, a1) is the anchor's side and mean / std
// d's normalisation: the same instructions as delta_core.h's decode give its clamped delta and the decoded size again.
template <bool GRAD>
__device__ __forceinline__ float ga_axis(float o0, float o1, float g0, float g1, float w_c, float w_s, float a0, float a1,
                                         float d, float mean, float std, const GlossArgs& A, float* grad) {
  const float pctr = __fmul_rn(__fadd_rn(o0, o1), 0.5f), psz = __fadd_rn(__fsub_rn(o1, o0), 1.0f);
  const float tctr = __fmul_rn(__fadd_rn(g0, g1), 0.5f), tsz = __fadd_rn(__fsub_rn(g1, g0), 1.0f);
  const float pe = __fadd_rn(psz, A.eps), te = __fadd_rn(tsz, A.eps);
  const float ra = __fdiv_rn(tsz, pe), rb = __fdiv_rn(psz, te);
  const float ls = __fsub_rn(1.f, fminf(ra, rb));
  if (GRAD) {
    const float ds = __fadd_rn(__fmul_rn(d, std), mean);
    const float dcl = fminf(fmaxf(ds, -A.max_ratio), A.max_ratio);
    const float gs = __fmul_rn(__fadd_rn(__fsub_rn(a1, a0), 1.0f), expf(dcl));
    // d ls / d psz = -d min(ra, rb); a tie takes half of each, as torch.min's backward does
    const float da = -__fdiv_rn(ra, pe), db = __fdiv_rn(1.f, te);
    const float dmin = ra < rb ? da : (ra > rb ? db : __fmul_rn(0.5f, __fadd_rn(da, db)));
    if (!(ds >= -A.max_ratio && ds <= A.max_ratio)) {          // torch.clamp's backward
      *grad = 0.f;
      return 0.f;
    }
    const float k = ga_shape_knee<true>(ls, A.beta, A.half_beta);
    *grad = __fmul_rn(__fmul_rn(__fmul_rn(w_s, k), -dmin), __fmul_rn(gs, std));
    return 0.f;
  }
  const float ad2 = __fmul_rn(2.f, fabsf(__fsub_rn(tctr, pctr)));
  const float lc = __fsub_rn(1.f, fmaxf(__fdiv_rn(__fsub_rn(tsz, ad2), __fadd_rn(__fadd_rn(tsz, ad2), A.eps)), 0.f));
  return __fadd_rn(__fmul_rn(w_c, ga_shape_knee<false>(lc, A.beta, A.half_beta)),
                   __fmul_rn(w_s, ga_shape_knee<false>(ls, A.beta, A.half_beta)));
}

template <int DT, bool GRAD>
__global__ __launch_bounds__(LT) void ga_loss_kernel(const GlossArgs A, const float* __restrict__ g,
                                                     const float* __restrict__ norm, double* __restrict__ partials) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  __shared__ double red[LWAVES][GPART];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float s_loc = 0.f, s_shape = 0.f;
  if (GRAD) {
    s_loc = __fdiv_rn(g[0], norm[0]);
    s_shape = __fdiv_rn(g[1], norm[1]);
  }
  double acc_loc = 0.0, acc_shape = 0.0;
  for (int64_t g0 = (int64_t)blockIdx.x * LT; g0 < A.nchunks; g0 += (int64_t)gridDim.x * LT) {
    const int64_t gc = g0 + tid;
    for (int s = 0; s < A.L; ++s) {                          // s is uniform
      const HeadSeg& S = A.seg[s];
      if (S.chunk0 + S.nchunks <= g0 || S.chunk0 >= g0 + LT) continue;
      if (gc >= S.chunk0 && gc < S.chunk0 + S.nchunks)
        acc_loc += ga_loc_chunk<DT, GRAD>(S, A, (uint32_t)(gc - S.chunk0), s_loc);
    }
  }
  for (int l = 0; l < A.L; ++l) {                            // uniform
    const GhLevel& V = A.lv[l];
    const int HW = V.HW, total = A.B * HW;
    for (int q0 = blockIdx.x * LT; q0 < total; q0 += gridDim.x * LT) {
      const int q = q0 + tid;
      if (q >= total) continue;
      const int b = q / HW, p = q - b * HW;
      const int64_t pt = (int64_t)b * A.N + V.off + p;
      float dgw = 0.f, dgh = 0.f;
      if (A.bw[pt * 4] > 0.f) {
        const f32x4_t w = *(const f32x4_t*)(A.bw + pt * 4);
        const f32x4_t an = *(const f32x4_t*)(A.anchors + pt * 4);
        const f32x4_t gt = *(const f32x4_t*)(A.gts + pt * 4);
        const float dw = E::ld(((const T*)V.shape)[ga_shape_index(V, b, p, 0)]);
        const float dh = E::ld(((const T*)V.shape)[ga_shape_index(V, b, p, 1)]);
        const f32x4_t o = decode_box(an, (f32x4_t){0.f, 0.f, dw, dh}, A.means, A.stds, A.max_ratio, -1, -1);
        const float vx = ga_axis<GRAD>(o[0], o[2], gt[0], gt[2], w[0], w[2], an[0], an[2], dw, A.means[2], A.stds[2], A,
                                       &dgw);
        const float vy = ga_axis<GRAD>(o[1], o[3], gt[1], gt[3], w[1], w[3], an[1], an[3], dh, A.means[3], A.stds[3], A,
                                       &dgh);
        if (GRAD) {
          dgw = __fmul_rn(dgw, s_shape);
          dgh = __fmul_rn(dgh, s_shape);
        } else {
          acc_shape += (double)vx;
          acc_shape += (double)vy;
        }
      }
      if (GRAD) {
        ((T*)V.dshape)[ga_shape_index(V, b, p, 0)] = E::st(dgw);
        ((T*)V.dshape)[ga_shape_index(V, b, p, 1)] = E::st(dgh);
      }
    }
  }
  if (GRAD) return;
  acc_loc = wave_sum(acc_loc);
  acc_shape = wave_sum(acc_shape);
  if (lane == 0) {
    red[wave][0] = acc_loc;
    red[wave][1] = acc_shape;
  }
  __syncthreads();
  if (tid < GPART) {
    double s = 0.0;
    for (int w = 0; w < LWAVES; ++w) s += red[w][tid];
    partials[(size_t)blockIdx.x * GPART + tid] = s;
  }
}

struct AvgArgs {
  const int32_t* a;
  const int32_t* b;
  int32_t na, nb, mode;
  float value;
};

// last launch: the partials in index order, the divisors, one rounding each
__global__ __launch_bounds__(LMAX_BLOCKS) void ga_loss_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                       float loc_avg, const AvgArgs V,
                                                                       float* __restrict__ losses,
                                                                       float* __restrict__ norm) {
  __shared__ double stage[LMAX_BLOCKS][GPART];
  const int t = threadIdx.x;
  if (t < nparts) {
    stage[t][0] = partials[(size_t)t * GPART + 0];
    stage[t][1] = partials[(size_t)t * GPART + 1];
  }
  __syncthreads();
  if (t != 0) return;
  double s0 = 0.0, s1 = 0.0;
  for (int i = 0; i < nparts; ++i) {
    s0 += stage[i][0];
    s1 += stage[i][1];
  }
  float avg = V.value;
  if (V.mode == 1) {
    long long n = 0;
    for (int i = 0; i < V.na; ++i) n += V.a[i];
    for (int i = 0; i < V.nb; ++i) n += V.b[i];
    avg = (float)(n < 1 ? 1ll : n);
  }
  losses[0] = (float)(s0 / (double)loc_avg);
  losses[1] = (float)(s1 / (double)avg);
  norm[0] = loc_avg;
  norm[1] = avg;
}

struct GlossPlan {
  GlossArgs A;
  int blocks;
};

int ga_check_dtype(const char* who, int dtype) {
  TDN_CHECK(dtype == TDN_F32 || dtype == TDN_BF16 || dtype == TDN_F16, "%s: dtype %d", who, dtype);
  return 0;
}

// the head tensors of every level; *items = the largest B * H*W of a level
int gh_levels(const char* who, const tdn_ga_level* levels, int L, int B, const GaGeo& G, GhLevel* lv, int64_t* items) {
  *items = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_ga_level& v = levels[l];
    const int64_t HW = (int64_t)v.H * v.W;
    TDN_CHECK((int64_t)B * 2 * HW < (1ll << 31), "%s: level %d holds 2^31 elements or more", who, l);
    TDN_CHECK((v.shape_nhwc | 1) == 1, "%s: level %d: the layout flag must be 0 or 1", who, l);
    lv[l].loc = v.loc;
    lv[l].shape = v.shape;
    lv[l].dloc = v.dloc;
    lv[l].dshape = v.dshape;
    lv[l].HW = (int)HW;
    lv[l].off = G.off[l];
    lv[l].shape_nhwc = v.shape_nhwc;
    if ((int64_t)B * HW > *items) *items = (int64_t)B * HW;
  }
  return 0;
}

int gloss_plan(const char* who, const tdn_ga_level* levels, int L, int B, const tdn_ga_loss_config* cfg,
               GlossPlan* out) {
  GaGeo G;
  if (ga_geo(who, levels, L, false, &G) != 0) return -1;
  TDN_CHECK(cfg, "%s: NULL config", who);
  if (tdn_check_batch(who, B) != 0 || ga_check_dtype(who, cfg->dtype) != 0) return -1;
  TDN_CHECK(cfg->gamma >= 0.f && cfg->gamma - cfg->gamma == 0.f && cfg->alpha >= 0.f && cfg->alpha <= 1.f,
            "%s: focal loss needs finite gamma >= 0 and alpha in [0, 1]", who);
  TDN_CHECK(cfg->beta > 0.f && cfg->beta < INFINITY, "%s: beta must be finite and > 0", who);
  TDN_CHECK(cfg->eps > 0.f && cfg->eps < 1.f, "%s: eps must be in (0, 1)", who);
  TDN_CHECK(cfg->loc_avg_factor > 0.f && cfg->loc_avg_factor < INFINITY, "%s: loc_avg_factor must be finite and > 0",
            who);
  for (int e = 0; e < 4; ++e)
    TDN_CHECK(cfg->means[e] - cfg->means[e] == 0.f && cfg->stds[e] - cfg->stds[e] == 0.f,
              "%s: anchoring means / stds must be finite", who);
  memset(out, 0, sizeof(*out));
  GlossArgs& A = out->A;
  A.L = L;
  A.B = B;
  A.N = G.N;
  A.means = host_f4(cfg->means);
  A.stds = host_f4(cfg->stds);
  A.max_ratio = (float)fabs(log(1e-6));            // as tdn_delta2bbox: in double, rounded to fp32
  A.beta = cfg->beta;
  A.half_beta = (float)(0.5 * (double)cfg->beta);  // exact: a power of two times an fp32
  A.eps = cfg->eps;
  A.P.focal = 1;
  A.P.gamma = cfg->gamma;
  A.P.alpha = cfg->alpha;
  A.P.one_minus_alpha = 1.f - cfg->alpha;
  int64_t items = 0;
  if (gh_levels(who, levels, L, B, G, A.lv, &items) != 0) return -1;
  const int V = cfg->dtype == TDN_F32 ? 4 : 8;
  int64_t chunks = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t HW = A.lv[l].HW, n = (int64_t)B * HW;
    HeadSeg& S = A.seg[l];
    S.n = (uint32_t)n;
    S.nchunks = (uint32_t)((n + V - 1) / V);
    S.chunk0 = chunks;
    S.Ch = 1;
    S.HW = (int32_t)HW;
    S.off = G.off[l];
    chunks += S.nchunks;
  }
  A.nchunks = chunks;
  out->blocks = tdn_grid_1d(chunks > items ? chunks : items, LT, LMAX_BLOCKS);
  return 0;
}

int gloss_pointers(const char* who, const tdn_ga_level* levels, int L, bool grad, GlossArgs* A,
                   const int64_t* loc_targets, const float* loc_weights, const float* bbox_anchors,
                   const float* bbox_gts, const float* bbox_weights) {
  TDN_CHECK(loc_targets && loc_weights && bbox_anchors && bbox_gts && bbox_weights, "%s: NULL targets", who);
  for (int l = 0; l < L; ++l) {
    const tdn_ga_level& v = levels[l];
    TDN_CHECK(v.loc && v.shape && (!grad || (v.dloc && v.dshape)), "%s: level %d has a NULL pointer", who, l);
    HeadSeg& S = A->seg[l];
    S.x = v.loc;
    S.dx = v.dloc;
    S.vec = (((uintptr_t)v.loc | (grad ? (uintptr_t)v.dloc : 0)) & 15) == 0;
  }
  A->loc_targets = loc_targets;
  A->loc_weights = loc_weights;
  A->anchors = bbox_anchors;
  A->gts = bbox_gts;
  A->bw = bbox_weights;
  return 0;
}

int ga_check_avg(const char* who, const tdn_loss_avg* avg, AvgArgs* out) {
  TDN_CHECK(avg != nullptr, "%s: NULL avg", who);
  TDN_CHECK(avg->mode == 0 || avg->mode == 1, "%s: avg mode %d", who, avg->mode);
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

#define GLOSS_LAUNCH(GRAD, dtype, grid, st, ...)                                                                     \
  do {                                                                                                               \
    if ((dtype) == TDN_F32) TDN_LAUNCH((ga_loss_kernel<TDN_F32, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);         \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((ga_loss_kernel<TDN_F16, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);    \
    else TDN_LAUNCH((ga_loss_kernel<TDN_BF16, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);                           \
  } while (0)


// ---- guided RPN proposals --------------------------------------------------------------------------------------------------
// tdn_rpn_proposals' pipeline (proposal.hip) with one anchor per location, anchors that differ per image
// and a location mask.  Launch 1 is this file's: rpn_topk_decode_kernel's steps with a masked key fetch and the
// per-image anchor row; it fills the same workspace, and launches 2-4 are proposal.hip's own (proposal_host.h).  A
// masked-out location gets key 0, below order_key of every logit that is not a NaN, so it sorts behind every location
// that is in, and the rows of key 0 are dropped after the sort: the level keeps the min(nms_pre, locations in) highest.
struct GpArgs {
  int L, per_img, N;
  float min_size, max_ratio;
  f32x4_t means, stds;
  const float* anchors;            // [B][N][4]
  const uint8_t* mask;             // [B][N]
  const void* logits[TDN_RPN_MAX_LEVELS];
  const void* deltas[TDN_RPN_MAX_LEVELS];
  int64_t ls[TDN_RPN_MAX_LEVELS][4], ds[TDN_RPN_MAX_LEVELS][4];
  int dtype[TDN_RPN_MAX_LEVELS], W[TDN_RPN_MAX_LEVELS];
  int n[TDN_RPN_MAX_LEVELS], cap[TDN_RPN_MAX_LEVELS], cap_off[TDN_RPN_MAX_LEVELS], aoff[TDN_RPN_MAX_LEVELS];
};

__device__ __forceinline__ float gp_load(const void* p, int dtype, int64_t off) {
  if (dtype == TDN_F32) return ((const float*)p)[off];
  return __uint_as_float((uint32_t)((const uint16_t*)p)[off] << 16);   // bf16 -> fp32 is exact
}

// logit keys of one (image, level): location i = y*W + x -> element (b, 0, y, x) through the strides; 0 where masked out
struct GpFetch {
  const void* p;
  int64_t base, sh, sw;
  int dtype, W;
  const uint8_t* m;                // the (image, level)'s mask bytes
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
    int y = i0 / W, x = i0 - (i0 / W) * W;
#pragma unroll
    for (int e = 0; e < TK_PER; ++e) {
      if (e < cnt) kk[e] = m[i0 + e] ? order_key(gp_load(p, dtype, base + y * sh + x * sw)) : 0u;
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
  }
};

constexpr int GP_SEG_MAX = TDN_NMS_SEG_MAX;
constexpr size_t GP_TOPK_LDS = (size_t)GP_SEG_MAX * 8 + TK_BINS * 4 + TK_MISC * 4;            // 41.2 KB

__global__ __launch_bounds__(1024) void ga_topk_decode_kernel(const GpArgs P, const int32_t* __restrict__ img_shapes,
                                                              f32x4_t* seg_box, uint32_t* seg_key, int* seg_aidx,
                                                              int* seg_start, int* seg_count) {
  extern __shared__ __attribute__((aligned(16))) u64 smem[];
  u64* skeys = smem;                                  // [GP_SEG_MAX]
  int* hist = (int*)(smem + GP_SEG_MAX);              // [TK_BINS]
  int* misc = hist + TK_BINS;                         // [TK_MISC]
  const int tid = threadIdx.x;
  const int s = blockIdx.x, b = s / P.L, l = s - (s / P.L) * P.L;
  const int n = P.n[l], W = P.W[l];
  const int start = b * P.per_img + P.cap_off[l];
  const int64_t row0 = (int64_t)b * P.N + P.aoff[l];  // the level's first location in the image's anchors and mask
  const GpFetch F{P.logits[l], b * P.ls[l][0], P.ls[l][2], P.ls[l][3], P.dtype[l], W, P.mask + row0};
  const int m = block_topk(F, n, P.cap[l], skeys, hist, misc);
  // decode the selected rows in key order; a thread takes `per` consecutive rows, so one scan keeps the order
  const int ih = img_shapes[2 * b], iw = img_shapes[2 * b + 1];
  const int per = (m + BLK - 1) / BLK;                // <= 4
  const int64_t* ds = P.ds[l];
  f32x4_t box[GP_SEG_MAX / BLK];
  uint32_t key[GP_SEG_MAX / BLK];
  int idx[GP_SEG_MAX / BLK];
  int ok = 0;
#pragma unroll
  for (int e = 0; e < GP_SEG_MAX / BLK; ++e) {
    const int p = tid * per + e;
    key[e] = 0u;
    idx[e] = -1;
    if (e < per && p < m) {
      const u64 c = skeys[p];
      key[e] = (uint32_t)(c >> 32);
      if (key[e] != 0u) {                             // a location that is in
        const int i = (int)~(uint32_t)c;
        const int y = i / W, x = i - (i / W) * W;
        const int64_t o = b * ds[0] + y * ds[2] + x * ds[3];
        f32x4_t d;
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = gp_load(P.deltas[l], P.dtype[l], o + j * ds[1]);
        box[e] = decode_box(*(const f32x4_t*)(P.anchors + (row0 + i) * 4), d, P.means, P.stds, P.max_ratio, ih, iw);
        bool keep = true;
        if (P.min_size > 0.f)
          keep = !(__fadd_rn(__fsub_rn(box[e][2], box[e][0]), 1.0f) < P.min_size ||
                   __fadd_rn(__fsub_rn(box[e][3], box[e][1]), 1.0f) < P.min_size);
        if (keep) {
          idx[e] = i;
          ++ok;
        }
      }
    }
  }
  int total;
  int q = start + block_excl_scan(ok, misc, &total);
#pragma unroll
  for (int e = 0; e < GP_SEG_MAX / BLK; ++e)
    if (idx[e] >= 0) {
      seg_box[q] = box[e];
      seg_key[q] = key[e];
      seg_aidx[q] = P.aoff[l] + idx[e];
      ++q;
    }
  if (tid == 0) {
    seg_start[s] = start;
    seg_count[s] = total;
  }
}

// the checks of the guided entry point that tdn_rpn_proposals' plan does not make, and launch 1's arguments; `lv`
// receives the levels as the plan wants them (a non-NULL anchors pointer per level)
int gp_plan(const char* who, const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg,
            const float* anchors, tdn_rpn_level* lv, GpArgs* out) {
  TDN_CHECK(levels && cfg, "%s: NULL levels / config", who);
  TDN_CHECK(nlevels >= 1 && nlevels <= TDN_RPN_MAX_LEVELS, "%s: 1..%d levels", who, TDN_RPN_MAX_LEVELS);
  if (tdn_check_batch(who, B) != 0) return -1;
  GpArgs& P = *out;
  memset(&P, 0, sizeof(P));
  P.L = nlevels;
  P.min_size = cfg->min_bbox_size;
  P.max_ratio = (float)fabs(log(16.0 / 1000.0));     // as tdn_rpn_proposals: in double, rounded to fp32
  P.means = host_f4(cfg->means);
  P.stds = host_f4(cfg->stds);
  int64_t per_img = 0, aoff = 0;
  for (int l = 0; l < nlevels; ++l) {
    const tdn_rpn_level& v = levels[l];
    TDN_CHECK(v.A == 1, "%s: level %d: a guided head has one anchor per location, A=%d", who, l, v.A);
    TDN_CHECK(v.H >= 1 && v.W >= 1, "%s: level %d is %d x %d", who, l, v.H, v.W);
    const int64_t n = (int64_t)v.H * v.W;
    const int64_t cap = cfg->nms_pre > 0 ? (n < cfg->nms_pre ? n : cfg->nms_pre) : n;
    lv[l] = v;
    lv[l].anchors = anchors ? anchors : (const float*)lv;          // the plan only asks that it is not NULL
    P.logits[l] = v.logits;
    P.deltas[l] = v.deltas;
    memcpy(P.ls[l], v.logit_strides, sizeof(P.ls[l]));
    memcpy(P.ds[l], v.delta_strides, sizeof(P.ds[l]));
    P.dtype[l] = v.dtype;
    P.W[l] = v.W;
    P.n[l] = (int)n;
    P.cap[l] = (int)cap;
    P.cap_off[l] = (int)per_img;
    P.aoff[l] = (int)aoff;
    per_img += cap;
    aoff += n;
    TDN_CHECK(aoff <= TDN_TARGET_MAX_BOXES, "%s: more than %d locations per image", who, TDN_TARGET_MAX_BOXES);
  }
  P.per_img = (int)per_img;
  P.N = (int)aoff;
  return 0;
}

}  // namespace

// ---- entry points ----------------------------------------------------------------------------------------------------------
extern "C" int tdn_ga_loc_target(const tdn_ga_level* levels, int nlevels, int B, const float* gt,
                                 const int32_t* gt_counts, int G, const tdn_ga_loc_config* cfg, int64_t* loc_targets,
                                 float* loc_weights, void* stream) {
  const char* who = "tdn_ga_loc_target";
  GlArgs A;
  memset(&A, 0, sizeof(A));
  if (ga_geo(who, levels, nlevels, true, &A.G) != 0 || ga_check_gt(who, B, G) != 0) return -1;
  TDN_CHECK(cfg, "%s: NULL config", who);
  for (int k = 0; k + 1 < nlevels; ++k) {
    TDN_CHECK(cfg->area_thr[k] > 0.f && cfg->area_thr[k] < INFINITY && (k == 0 || cfg->area_thr[k] > cfg->area_thr[k - 1]),
              "%s: the area thresholds must be finite, positive and ascending", who);
    A.thr[k] = cfg->area_thr[k];
  }
  const float r4[4] = {cfg->center_r, cfg->center_c, cfg->ignore_r, cfg->ignore_c};
  for (int e = 0; e < 4; ++e) TDN_CHECK(r4[e] >= 0.f && r4[e] <= 1.f, "%s: a region ratio is outside [0, 1]", who);
  A.rc = cfg->center_r;
  A.cc = cfg->center_c;
  A.ri = cfg->ignore_r;
  A.ci = cfg->ignore_c;
  A.NG = G;
  TDN_CHECK(G == 0 || (gt && gt_counts), "%s: NULL ground truths", who);
  TDN_CHECK(loc_targets && loc_weights, "%s: NULL output", who);
  TDN_LAUNCH(ga_loc_target_kernel, dim3((A.G.N + GT_ - 1) / GT_, B), dim3(GT_), 0, (hipStream_t)stream, A, gt, gt_counts,
             loc_targets, loc_weights);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_ga_shape_target_workspace_bytes(int B, int N, int G) {
  if (gs_check_dims("tdn_ga_shape_target_workspace_bytes", B, N, G, 1) != 0) return -1;
  return gs_layout(B, N, G, nullptr).bytes;
}

extern "C" int tdn_ga_shape_target(const float* approxs, int A, const float* squares, const uint8_t* valid,
                                   int64_t valid_stride, const float* gt, const int32_t* gt_counts,
                                   const int32_t* img_shapes, int B, int N, int G, const tdn_target_config* cfg,
                                   int sampling, const int32_t* keys, float* bbox_anchors, float* bbox_gts,
                                   float* bbox_weights, int32_t* num_pos, int32_t* num_neg, int32_t* assigned,
                                   float* max_overlaps, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_ga_shape_target";
  if (gs_check_dims(who, B, N, G, A) != 0) return -1;
  TDN_CHECK(cfg, "%s: NULL config", who);
  TDN_CHECK(cfg->pos_iou_thr == cfg->pos_iou_thr && cfg->neg_iou_thr == cfg->neg_iou_thr &&
                cfg->min_pos_iou == cfg->min_pos_iou, "%s: NaN threshold", who);
  TDN_CHECK(valid_stride == 0 || valid_stride >= (int64_t)N * A, "%s: bad valid_stride", who);
  TDN_CHECK(approxs && squares && gt_counts && (G == 0 || gt), "%s: NULL pointer", who);
  TDN_CHECK(bbox_anchors && bbox_gts && bbox_weights && num_pos && num_neg && assigned && max_overlaps,
            "%s: NULL output", who);
  TDN_CHECK(cfg->allowed_border < 0 || img_shapes, "%s: allowed_border >= 0 needs img_shapes", who);
  const GsWs w = gs_layout(B, N, G, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  GsArgs S;
  memset(&S, 0, sizeof(S));
  S.approxs = approxs;
  S.valid = valid;
  S.vstride = valid_stride;
  S.img_shapes = img_shapes;
  S.border = img_shapes ? cfg->allowed_border : -1;
  S.gt = gt;
  S.gt_counts = gt_counts;
  S.N = N;
  S.G = G;
  S.A = A;
  S.all = cfg->gt_max_assign_all != 0;
  S.pos_thr = cfg->pos_iou_thr;
  S.neg_thr = cfg->neg_iou_thr;
  S.min_pos = cfg->min_pos_iou;
  if (const int rc = tdn_target_clear(w.colmax, w.first, w.words, stream)) return rc;
  const dim3 grid((N + P1_THREADS * P1_PER - 1) / (P1_THREADS * P1_PER), B);
  GS_LAUNCH(ga_assign_pass1_kernel, A, grid, st, S, assigned, max_overlaps, w.colmax);
  TDN_LAUNCH_CHECK();
  if (G > 0) {
    GS_LAUNCH(ga_assign_pass2_kernel, A, grid, st, S, assigned, (const uint32_t*)w.colmax, w.first);
    TDN_LAUNCH_CHECK();
    if (!S.all && tdn_target_assign_first(w.first, gt_counts, B, N, G, assigned, stream) != 0) return -2;
  }
  if (sampling) {
    if (tdn_sample_assigned(assigned, B, N, cfg, keys, w.pos_mask, w.neg_mask, num_pos, num_neg, stream) != 0) return -1;
  } else {
    TDN_LAUNCH(ga_take_all_kernel, dim3(B), dim3(1024), 0, st, (const int32_t*)assigned, N, w.pos_mask, w.neg_mask,
               num_pos, num_neg);
    TDN_LAUNCH_CHECK();
  }
  TDN_LAUNCH(ga_shape_fill_kernel, dim3(tdn_grid_1d(N, 256, 2048), B), dim3(256), 0, st, squares, gt, N, G,
             (const int32_t*)assigned, (const uint8_t*)w.pos_mask, bbox_anchors, bbox_gts, bbox_weights);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_guided_anchors(const tdn_ga_level* levels, int nlevels, int B, int dtype, const float* squares,
                                  const float* means4, const float* stds4, int use_loc, float loc_thr_logit,
                                  float* anchors, uint8_t* loc_mask, void* stream) {
  const char* who = "tdn_guided_anchors";
  GdArgs A;
  memset(&A, 0, sizeof(A));
  if (ga_geo(who, levels, nlevels, false, &A.G) != 0) return -1;
  if (tdn_check_batch(who, B) != 0 || ga_check_dtype(who, dtype) != 0) return -1;
  TDN_CHECK(squares && means4 && stds4 && anchors && loc_mask, "%s: NULL pointer", who);
  TDN_CHECK(!use_loc || loc_thr_logit == loc_thr_logit, "%s: NaN threshold", who);
  int64_t items;
  if (gh_levels(who, levels, nlevels, B, A.G, A.lv, &items) != 0) return -1;
  for (int l = 0; l < nlevels; ++l)
    TDN_CHECK(levels[l].shape && (!use_loc || levels[l].loc), "%s: level %d has a NULL pointer", who, l);
  A.means = host_f4(means4);
  A.stds = host_f4(stds4);
  A.max_ratio = (float)fabs(log(1e-6));            // as tdn_delta2bbox: in double, rounded to fp32
  A.thr = loc_thr_logit;
  A.use_loc = use_loc ? 1 : 0;
  const dim3 grid((A.G.N + GT_ - 1) / GT_, B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TDN_F32) TDN_LAUNCH(guided_anchors_kernel<TDN_F32>, grid, dim3(GT_), 0, st, A, squares, anchors, loc_mask);
  else if (dtype == TDN_F16)
    TDN_LAUNCH(guided_anchors_kernel<TDN_F16>, grid, dim3(GT_), 0, st, A, squares, anchors, loc_mask);
  else TDN_LAUNCH(guided_anchors_kernel<TDN_BF16>, grid, dim3(GT_), 0, st, A, squares, anchors, loc_mask);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_ga_loss_workspace_bytes(const tdn_ga_level* levels, int nlevels, int B,
                                               const tdn_ga_loss_config* cfg) {
  GlossPlan p;
  if (gloss_plan("tdn_ga_loss_workspace_bytes", levels, nlevels, B, cfg, &p) != 0) return -1;
  return align256((int64_t)p.blocks * GPART * (int64_t)sizeof(double));
}

extern "C" int tdn_ga_loss_fwd(const tdn_ga_level* levels, int nlevels, int B, const tdn_ga_loss_config* cfg,
                               const int64_t* loc_targets, const float* loc_weights, const float* bbox_anchors,
                               const float* bbox_gts, const float* bbox_weights, const tdn_loss_avg* avg, float* losses,
                               float* norm, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_ga_loss_fwd";
  GlossPlan p;
  AvgArgs V;
  if (gloss_plan(who, levels, nlevels, B, cfg, &p) != 0 || ga_check_avg(who, avg, &V) != 0) return -1;
  if (gloss_pointers(who, levels, nlevels, false, &p.A, loc_targets, loc_weights, bbox_anchors, bbox_gts,
                     bbox_weights) != 0)
    return -1;
  TDN_CHECK(losses && norm, "%s: NULL output", who);
  if (tdn_check_ws(who, workspace, workspace_bytes, align256((int64_t)p.blocks * GPART * (int64_t)sizeof(double))) != 0)
    return -1;
  double* partials = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  GLOSS_LAUNCH(false, cfg->dtype, dim3(p.blocks), st, p.A, (const float*)nullptr, (const float*)nullptr, partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(ga_loss_finalize_kernel, dim3(1), dim3(LMAX_BLOCKS), 0, st, (const double*)partials, p.blocks,
             cfg->loc_avg_factor, V, losses, norm);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_ga_loss_bwd(const tdn_ga_level* levels, int nlevels, int B, const tdn_ga_loss_config* cfg,
                               const int64_t* loc_targets, const float* loc_weights, const float* bbox_anchors,
                               const float* bbox_gts, const float* bbox_weights, const float* g, const float* norm,
                               void* stream) {
  const char* who = "tdn_ga_loss_bwd";
  GlossPlan p;
  if (gloss_plan(who, levels, nlevels, B, cfg, &p) != 0) return -1;
  if (gloss_pointers(who, levels, nlevels, true, &p.A, loc_targets, loc_weights, bbox_anchors, bbox_gts,
                     bbox_weights) != 0)
    return -1;
  TDN_CHECK(g && norm, "%s: NULL cotangent / divisors", who);
  GLOSS_LAUNCH(true, cfg->dtype, dim3(p.blocks), (hipStream_t)stream, p.A, g, norm, (double*)nullptr);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_ga_rpn_proposals_workspace_bytes(const tdn_rpn_level* levels, int nlevels, int B,
                                                        const tdn_rpn_config* cfg) {
  tdn_rpn_level lv[TDN_RPN_MAX_LEVELS];
  GpArgs P;
  tdn_rpn_ws w;
  if (gp_plan("tdn_ga_rpn_proposals_workspace_bytes", levels, nlevels, B, cfg, nullptr, lv, &P) != 0) return -1;
  if (tdn_rpn_ws_layout(lv, nlevels, B, cfg, nullptr, &w) != 0) return -1;
  return w.bytes;
}

extern "C" int tdn_ga_rpn_proposals(const tdn_rpn_level* levels, int nlevels, int B, const float* anchors,
                                    const uint8_t* loc_mask, const int32_t* img_shapes, const tdn_rpn_config* cfg,
                                    float* proposals, int64_t* anchor_idx, int32_t* counts, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_ga_rpn_proposals";
  tdn_rpn_level lv[TDN_RPN_MAX_LEVELS];
  GpArgs P;
  tdn_rpn_ws w;
  TDN_CHECK(anchors && loc_mask && img_shapes && proposals && anchor_idx && counts && workspace, "%s: NULL pointer", who);
  if (gp_plan(who, levels, nlevels, B, cfg, anchors, lv, &P) != 0) return -1;
  if (tdn_rpn_ws_layout(lv, nlevels, B, cfg, workspace, &w) != 0) return -1;   // the plan's checks and limits
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  P.anchors = anchors;
  P.mask = loc_mask;
  TDN_LAUNCH(ga_topk_decode_kernel, dim3(B * nlevels), dim3(BLK), GP_TOPK_LDS, (hipStream_t)stream, P, img_shapes,
             w.seg_box, w.seg_key, w.seg_aidx, w.seg_start, w.seg_count);
  TDN_LAUNCH_CHECK();
  return tdn_rpn_nms_merge(lv, nlevels, B, cfg, &w, proposals, anchor_idx, counts, stream);
}
