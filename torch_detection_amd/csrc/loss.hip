// Losses of the dense anchor heads (sigmoid BCE / focal + smooth L1) and of the RoI box head (softmax CE + smooth L1)
// with their gradients (gfx950; DESIGN.md §4e has the spec, tests/loss_ref.py restates it).
//
// Per-element work is fp32 with explicit __f*_rn arithmetic (this file is compiled with -ffp-contract=off); sums are
// fp64.  Which lane, wave and workgroup an element goes to depends on the shapes alone; a workgroup's partial goes to
// the workspace with a plain store and the last launch adds the partials in index order, so two runs agree bit for
// bit.  An element whose weight is exactly 0 is not evaluated.  No float atomics, no host synchronisation, no
// allocation; every launch goes through TDN_LAUNCH.
#include "loss_core.h"
#include <string.h>

namespace {

constexpr int LT = 1024;          // threads per workgroup: 16 waves, four per SIMD
constexpr int LWAVES = LT / 64;
constexpr int LMAX_BLOCKS = 256;  // one workgroup per CU at most: that many partials for the last launch
constexpr int PART = 4;           // doubles per partial: loss_cls, loss_bbox, rows with weight > 0, unused
constexpr int MAXSEG = HEAD_MAXSEG;

// ---- elementwise spec: the sigmoid classification terms are loss_core.h ----------------------------------------------
template <bool GRAD>
__device__ __forceinline__ float smooth_l1(float pred, float target, float beta) {
  const float d = __fsub_rn(pred, target);
  const float ad = fabsf(d);
  if (ad < beta) return GRAD ? __fdiv_rn(d, beta) : __fdiv_rn(__fmul_rn(__fmul_rn(0.5f, d), d), beta);
  if (GRAD) return d > 0.f ? 1.f : (d < 0.f ? -1.f : d);      // NaN stays NaN
  return __fsub_rn(ad, __fmul_rn(0.5f, beta));
}

// ---- block reduction of the fp64 accumulators (storage types and wave_sum: loss_core.h) -------------------------------
// lanes -> xor tree, waves -> wave 0 .. 15 in order; thread 0 stores the workgroup's partial
__device__ __forceinline__ void block_partial(double a0, double a1, double a2, double* __restrict__ partials) {
  __shared__ double red[LWAVES][3];
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  a2 = wave_sum(a2);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = a0;
    red[wave][1] = a1;
    red[wave][2] = a2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int w = 0; w < LWAVES; ++w) {
      s0 += red[w][0];
      s1 += red[w][1];
      s2 += red[w][2];
    }
    double* p = partials + (size_t)blockIdx.x * PART;
    p[0] = s0;
    p[1] = s1;
    p[2] = s2;
    p[3] = 0.0;
  }
}

// ---- dense heads ----------------------------------------------------------------------------------------------------
// The segments and their walk are loss_core.h's.  Chunk indices run through all segments; a workgroup takes 1024
// consecutive chunks per grid stride.
typedef HeadSeg DenseSeg;
struct DenseArgs {
  DenseSeg seg[MAXSEG];
  int32_t nseg;
  int64_t nchunks;
  const int64_t* labels;
  const float* lw;
  const float* bt;
  const float* bw;
  int32_t N, A, C;
  float beta;
  ClsParams P;
};

template <int DT, bool GRAD>
__device__ __forceinline__ double dense_chunk(const DenseSeg& S, const DenseArgs& A, uint32_t lc, float s_cls,
                                              float s_reg) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  const uint32_t m0 = lc * (uint32_t)V;
  const int cnt = (int)min((uint32_t)V, S.n - m0);
  const Vec<T, V> in = head_load<DT>(S, m0, cnt);
  Vec<T, V> out;
  // coordinates of the chunk's first element; the following elements advance them
  const int div = S.reg ? 4 : A.C;               // channels per anchor
  HeadPos P = head_pos(S, m0, div);
  int last_idx = -1;
  float last_w = 0.f;
  long long last_lab = 0;
  double sum = 0.0;                              // the chunk's elements in memory order
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float res = 0.f;
    if (e < cnt) {
      const int idx = (int)P.b * A.N + S.off + (int)P.p * A.A + P.a;     // < 64 * 2^20
      const int k = P.k;
      const float x = E::ld(in.v[e]);
      if (S.reg) {
        const float w = A.bw[(size_t)idx * 4 + k];
        if (w != 0.f) {
          const float v = smooth_l1<GRAD>(x, A.bt[(size_t)idx * 4 + k], A.beta);
          if (GRAD) res = __fmul_rn(__fmul_rn(w, v), s_reg);
          else sum += (double)__fmul_rn(w, v);
        }
      } else {
        if (idx != last_idx) {
          last_idx = idx;
          last_w = A.lw[idx];
          if (last_w != 0.f) last_lab = A.labels[idx];
        }
        if (last_w != 0.f) {
          const float v = cls_elem<GRAD>(x, last_lab == (long long)k + 1, A.P);
          if (GRAD) res = __fmul_rn(__fmul_rn(last_w, v), s_cls);
          else sum += (double)__fmul_rn(last_w, v);
        }
      }
      head_next(S, div, P);
    }
    if (GRAD) out.v[e] = E::st(res);
  }
  if (GRAD) head_store<DT>(S, m0, cnt, out);
  return sum;
}

template <int DT, bool GRAD>
__global__ __launch_bounds__(LT) void loss_dense_kernel(const DenseArgs A, const float* __restrict__ g,
                                                        const float* __restrict__ avg, double* __restrict__ partials) {
  float s_cls = 0.f, s_reg = 0.f;
  if (GRAD) {
    const float d = avg[0];
    s_cls = __fdiv_rn(g[0], d);
    s_reg = __fdiv_rn(g[1], d);
  }
  double acc_cls = 0.0, acc_reg = 0.0;
  for (int64_t g0 = (int64_t)blockIdx.x * LT; g0 < A.nchunks; g0 += (int64_t)gridDim.x * LT) {
    const int64_t gc = g0 + threadIdx.x;
    for (int s = 0; s < A.nseg; ++s) {                     // s is uniform: the segment comes through scalar loads
      const DenseSeg& S = A.seg[s];
      if (S.chunk0 + S.nchunks <= g0 || S.chunk0 >= g0 + LT) continue;
      if (gc >= S.chunk0 && gc < S.chunk0 + S.nchunks) {
        const double sum = dense_chunk<DT, GRAD>(S, A, (uint32_t)(gc - S.chunk0), s_cls, s_reg);
        acc_cls += S.reg ? 0.0 : sum;            // selects, not a branch: both accumulators stay in registers
        acc_reg += S.reg ? sum : 0.0;
      }
    }
  }
  if (!GRAD) block_partial(acc_cls, acc_reg, 0.0, partials);
}

// ---- last launch: partials in index order, divisor, one rounding ------------------------------------------------------
struct AvgArgs {
  const int32_t* a;
  const int32_t* b;
  int32_t na, nb, mode;
  float value;
};

__global__ __launch_bounds__(LMAX_BLOCKS) void loss_finalize_kernel(const double* __restrict__ partials, int nparts,
                                                                    const AvgArgs V, float* __restrict__ losses,
                                                                    float* __restrict__ avg_out) {
  __shared__ double stage[LMAX_BLOCKS][3];
  const int t = threadIdx.x;
  if (t < nparts) {
    stage[t][0] = partials[(size_t)t * PART + 0];
    stage[t][1] = partials[(size_t)t * PART + 1];
    stage[t][2] = partials[(size_t)t * PART + 2];
  }
  __syncthreads();
  if (t != 0) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < nparts; ++i) {
    s0 += stage[i][0];
    s1 += stage[i][1];
    s2 += stage[i][2];
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
      n = (long long)s2;                         // a count of rows: exact in fp64
    }
    avg = (float)(n < 1 ? 1ll : n);
  }
  losses[0] = (float)(s0 / (double)avg);
  losses[1] = (float)(s1 / (double)avg);
  avg_out[0] = avg;
}

// ---- RoI box head ---------------------------------------------------------------------------------------------------
// One wavefront per row; lane l holds columns l, l + 64, ... (at most 16).  S is added in fp64: lane-local in column
// order, then the xor tree, then rounded once to fp32.
constexpr int RCOLS = TDN_LOSS_MAX_CLASSES / 64;

struct RoiArgs {
  const void* cls;
  const void* reg;
  void* dcls;
  void* dreg;
  const int64_t* labels;
  const float* lw;
  const float* bt;
  const float* bw;
  int32_t R, C, reg_cols;
  float beta;
  BalancedL1 bal;                 // BALANCED instantiations only
};

template <int DT, bool GRAD, bool BALANCED>
__global__ __launch_bounds__(LT) void loss_roi_kernel(const RoiArgs A, const float* __restrict__ g,
                                                      const float* __restrict__ avg, double* __restrict__ partials) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float s_cls = 0.f, s_reg = 0.f;
  if (GRAD) {
    const float d = avg[0];
    s_cls = __fdiv_rn(g[0], d);
    s_reg = __fdiv_rn(g[1], d);
  }
  double acc_cls = 0.0, acc_reg = 0.0, acc_cnt = 0.0;
  const int C = A.C;
  for (int r = blockIdx.x * LWAVES + wave; r < A.R; r += gridDim.x * LWAVES) {
    const float w = A.lw[r];
    const long long lab = A.labels[r];
    if (!GRAD && lane == 0 && w > 0.f) acc_cnt += 1.0;
    const bool live = w != 0.f && lab >= 0 && lab < C;         // wave-uniform
    const int il = (int)lab;
    const T* xr = (const T*)A.cls + (size_t)r * C;
    T* dr = GRAD ? (T*)A.dcls + (size_t)r * C : nullptr;
    T* br = GRAD ? (T*)A.dreg + (size_t)r * A.reg_cols : nullptr;
    if (!live) {
      if (GRAD) {
        for (int c = lane; c < C; c += 64) dr[c] = E::st(0.f);
        for (int c = lane; c < A.reg_cols; c += 64) br[c] = E::st(0.f);
      }
      continue;
    }
    float x[RCOLS];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < RCOLS; ++j) {
      const int c = lane + 64 * j;
      x[j] = c < C ? E::ld(xr[c]) : -INFINITY;
      m = fmaxf(m, x[j]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    double sd = 0.0;
    float zl = 0.f;                                            // z of the label's column, on the lane that holds it
#pragma unroll
    for (int j = 0; j < RCOLS; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        const float z = __fsub_rn(x[j], m);
        x[j] = expf(z);
        sd += (double)x[j];
        if (c == il) zl = z;
      }
    }
    const float S = (float)wave_sum(sd);
    if (!GRAD) {
      if (lane == (il & 63)) acc_cls += (double)__fmul_rn(w, __fsub_rn(logf(S), zl));
    } else {
#pragma unroll
      for (int j = 0; j < RCOLS; ++j) {
        const int c = lane + 64 * j;
        if (c < C) {
          const float d = __fsub_rn(__fdiv_rn(x[j], S), c == il ? 1.f : 0.f);
          dr[c] = E::st(__fmul_rn(__fmul_rn(w, d), s_cls));
        }
      }
    }
    // box columns of the row's label (class-specific) or the four there are
    const int col0 = A.reg_cols == 4 ? 0 : 4 * il;
    if (GRAD) {
      for (int c = lane; c < A.reg_cols; c += 64)
        if (c < col0 || c >= col0 + 4) br[c] = E::st(0.f);
    }
    if (lane < 4) {
      const float bw = A.bw[(size_t)r * 4 + lane];
      float res = 0.f;
      if (bw != 0.f) {
        const float pred = E::ld(((const T*)A.reg)[(size_t)r * A.reg_cols + col0 + lane]);
        const float tgt = A.bt[(size_t)r * 4 + lane];
        const float v = BALANCED ? balanced_l1<GRAD>(pred, tgt, A.bal) : smooth_l1<GRAD>(pred, tgt, A.beta);
        if (GRAD) res = __fmul_rn(__fmul_rn(bw, v), s_reg);
        else acc_reg += (double)__fmul_rn(bw, v);
      }
      if (GRAD) br[col0 + lane] = E::st(res);
    }
  }
  if (!GRAD) block_partial(acc_cls, acc_reg, acc_cnt, partials);
}

// ---- host -----------------------------------------------------------------------------------------------------------
// the one workspace of this file: a partial per workgroup of the forward launch
struct PartialsWs { double* partials; int64_t bytes; };
PartialsWs partials_layout(int blocks, void* base) {   // a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<double>((int64_t)blocks * PART), c.off};
}

int check_avg(const char* who, const tdn_loss_avg* avg, bool roi, AvgArgs* out) {
  TDN_CHECK(avg != nullptr, "%s: NULL avg", who);
  TDN_CHECK(avg->mode == 0 || avg->mode == 1 || (roi && avg->mode == 2), "%s: avg mode %d", who, avg->mode);
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

// The shape half of the plan, all the size query needs: checks of everything the sizes depend on, the segment table
// without its pointers, the anchor and chunk totals.  Returns the number of workgroups, or -1 with the error set.
int dense_shape(const char* who, const tdn_loss_level* levels, int L, int B, const tdn_loss_config* cfg, DenseArgs* D) {
  TDN_CHECK(levels && cfg, "%s: NULL argument", who);
  TDN_CHECK(L >= 1 && L <= TDN_LOSS_MAX_LEVELS, "%s: %d levels (1..%d)", who, L, TDN_LOSS_MAX_LEVELS);
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(cfg->dtype == TDN_F32 || cfg->dtype == TDN_BF16 || cfg->dtype == TDN_F16, "%s: dtype %d", who, cfg->dtype);
  TDN_CHECK(cfg->num_anchors >= 1 && cfg->num_classes >= 1 && cfg->num_classes <= TDN_LOSS_MAX_CLASSES,
            "%s: A=%d, C=%d (C in 1..%d)", who, cfg->num_anchors, cfg->num_classes, TDN_LOSS_MAX_CLASSES);
  memset(D, 0, sizeof(*D));
  const int A = cfg->num_anchors, C = cfg->num_classes;
  int64_t chunk = 0;
  const int64_t N = head_segments(who, levels, L, B, cfg->dtype, A, C, D->seg, &chunk);
  if (N < 0) return -1;
  D->nseg = 2 * L;
  D->nchunks = chunk;
  D->N = (int32_t)N;
  D->A = A;
  D->C = C;
  const int64_t blocks = (chunk + LT - 1) / LT;
  return (int)(blocks < LMAX_BLOCKS ? blocks : LMAX_BLOCKS);
}

// The pointer half: the loss parameters and each segment's tensors.  Same return value.
int dense_plan(const char* who, const tdn_loss_level* levels, int L, int B, const tdn_loss_config* cfg, bool grad,
               DenseArgs* D) {
  const int blocks = dense_shape(who, levels, L, B, cfg, D);
  if (blocks < 0) return -1;
  TDN_CHECK(cfg->beta > 0.f && cfg->beta < INFINITY, "%s: beta must be finite and > 0", who);
  if (cfg->focal)
    TDN_CHECK(cfg->gamma >= 0.f && cfg->gamma < INFINITY && cfg->alpha >= 0.f && cfg->alpha <= 1.f,
              "%s: focal needs gamma >= 0 and alpha in [0, 1]", who);
  if (head_pointers(who, levels, L, grad, D->seg) != 0) return -1;
  D->beta = cfg->beta;
  D->P = {cfg->focal ? 1 : 0, cfg->gamma, cfg->alpha, 1.f - cfg->alpha};
  return blocks;
}

int roi_blocks(int R) {
  const int b = (R + LWAVES - 1) / LWAVES;
  return b < 1 ? 1 : (b < LMAX_BLOCKS ? b : LMAX_BLOCKS);
}

int check_roi(const char* who, int dtype, int R, int C, int reg_cols, float beta) {
  TDN_CHECK(dtype == TDN_F32 || dtype == TDN_BF16 || dtype == TDN_F16, "%s: dtype %d", who, dtype);
  TDN_CHECK(R >= 0 && R <= TDN_LOSS_MAX_ROWS, "%s: R=%d out of 0..%d", who, R, TDN_LOSS_MAX_ROWS);
  TDN_CHECK(C >= 1 && C <= TDN_LOSS_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_LOSS_MAX_CLASSES);
  TDN_CHECK(reg_cols == 4 || reg_cols == 4 * C, "%s: bbox_pred has %d columns, neither 4 nor 4C", who, reg_cols);
  TDN_CHECK(beta > 0.f && beta < INFINITY, "%s: beta must be finite and > 0", who);
  return 0;
}

// the knee, the two shape parameters and the host-formed constants of balanced L1
int balanced_params(const char* who, float beta, float alpha, float gamma, BalancedL1* P) {
  TDN_CHECK(alpha > 0.f && alpha < INFINITY && gamma > 0.f && gamma < INFINITY,
            "%s: balanced L1 needs finite alpha > 0 and gamma > 0", who);
  const double b = exp((double)gamma / (double)alpha) - 1.0;
  P->alpha = alpha;
  P->gamma = gamma;
  P->beta = beta;
  P->b = (float)b;
  P->alpha_over_b = (float)((double)alpha / b);
  P->outer_c = (float)((double)gamma / b - (double)alpha * (double)beta);
  P->knee_c = (float)((double)alpha * (1.0 - (double)beta));
  TDN_CHECK(P->b > 0.f && P->b < INFINITY && P->alpha_over_b > 0.f, "%s: gamma / alpha = %g leaves float range", who,
            (double)gamma / (double)alpha);
  return 0;
}

#define LOSS_LAUNCH_DT(kernel, GRAD, dtype, grid, st, ...)                                             \
  do {                                                                                                 \
    if ((dtype) == TDN_F32) TDN_LAUNCH((kernel<TDN_F32, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);    \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((kernel<TDN_F16, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__); \
    else TDN_LAUNCH((kernel<TDN_BF16, GRAD>), grid, dim3(LT), 0, st, __VA_ARGS__);                       \
  } while (0)

}  // namespace

extern "C" int64_t tdn_loss_dense_workspace_bytes(const tdn_loss_level* levels, int num_levels, int B,
                                                  const tdn_loss_config* cfg) {
  DenseArgs D;
  const int blocks = dense_shape("tdn_loss_dense_workspace_bytes", levels, num_levels, B, cfg, &D);
  return blocks < 0 ? -1 : partials_layout(blocks, nullptr).bytes;
}

extern "C" int tdn_loss_dense_fwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_loss_config* cfg,
                                  const int64_t* labels, const float* label_weights, const float* bbox_targets,
                                  const float* bbox_weights, const tdn_loss_avg* avg, float* losses, float* avg_out,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_loss_dense_fwd";
  DenseArgs D;
  AvgArgs V;
  const int blocks = dense_plan(who, levels, num_levels, B, cfg, false, &D);
  if (blocks < 0 || check_avg(who, avg, false, &V) != 0) return -1;
  TDN_CHECK(labels && label_weights && bbox_targets && bbox_weights && losses && avg_out && workspace,
            "%s: NULL pointer", who);
  const PartialsWs w = partials_layout(blocks, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  D.labels = labels;
  D.lw = label_weights;
  D.bt = bbox_targets;
  D.bw = bbox_weights;
  const float* none = nullptr;
  LOSS_LAUNCH_DT(loss_dense_kernel, false, cfg->dtype, dim3(blocks), stream, D, none, none, w.partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(loss_finalize_kernel, dim3(1), dim3(LMAX_BLOCKS), 0, stream, (const double*)w.partials, blocks, V, losses,
             avg_out);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_loss_dense_bwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_loss_config* cfg,
                                  const int64_t* labels, const float* label_weights, const float* bbox_targets,
                                  const float* bbox_weights, const float* g, const float* avg_in, void* stream) {
  const char* who = "tdn_loss_dense_bwd";
  DenseArgs D;
  const int blocks = dense_plan(who, levels, num_levels, B, cfg, true, &D);
  if (blocks < 0) return -1;
  TDN_CHECK(labels && label_weights && bbox_targets && bbox_weights && g && avg_in, "%s: NULL pointer", who);
  D.labels = labels;
  D.lw = label_weights;
  D.bt = bbox_targets;
  D.bw = bbox_weights;
  double* none = nullptr;
  LOSS_LAUNCH_DT(loss_dense_kernel, true, cfg->dtype, dim3(blocks), stream, D, g, avg_in, none);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_loss_roi_workspace_bytes(int R) {
  if (R < 0 || R > TDN_LOSS_MAX_ROWS) return -1;
  return partials_layout(roi_blocks(R), nullptr).bytes;
}

namespace {

#define LOSS_LAUNCH_ROI(GRAD, BAL, dtype, grid, st, ...)                                                          \
  do {                                                                                                            \
    if ((dtype) == TDN_F32) TDN_LAUNCH((loss_roi_kernel<TDN_F32, GRAD, BAL>), grid, dim3(LT), 0, st, __VA_ARGS__); \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((loss_roi_kernel<TDN_F16, GRAD, BAL>), grid, dim3(LT), 0, st, __VA_ARGS__); \
    else TDN_LAUNCH((loss_roi_kernel<TDN_BF16, GRAD, BAL>), grid, dim3(LT), 0, st, __VA_ARGS__);                   \
  } while (0)

// bal: nullptr for smooth L1
int roi_fwd(const char* who, const BalancedL1* bal, const void* cls, const void* reg, int dtype, int R, int C,
            int reg_cols, const int64_t* labels, const float* label_weights, const float* bbox_targets,
            const float* bbox_weights, float beta, const tdn_loss_avg* avg, float* losses, float* avg_out,
            void* workspace, int64_t workspace_bytes, void* stream) {
  AvgArgs V;
  if (check_avg(who, avg, true, &V) != 0) return -1;
  TDN_CHECK(losses && avg_out && workspace, "%s: NULL pointer", who);
  TDN_CHECK(R == 0 || (cls && reg && labels && label_weights && bbox_targets && bbox_weights), "%s: NULL pointer", who);
  const int blocks = roi_blocks(R);
  const PartialsWs w = partials_layout(blocks, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  RoiArgs A;
  memset(&A, 0, sizeof(A));
  A.cls = cls;
  A.reg = reg;
  A.labels = labels;
  A.lw = label_weights;
  A.bt = bbox_targets;
  A.bw = bbox_weights;
  A.R = R;
  A.C = C;
  A.reg_cols = reg_cols;
  A.beta = beta;
  if (bal) A.bal = *bal;
  const float* none = nullptr;
  if (bal) LOSS_LAUNCH_ROI(false, true, dtype, dim3(blocks), stream, A, none, none, w.partials);
  else LOSS_LAUNCH_ROI(false, false, dtype, dim3(blocks), stream, A, none, none, w.partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(loss_finalize_kernel, dim3(1), dim3(LMAX_BLOCKS), 0, stream, (const double*)w.partials, blocks, V, losses,
             avg_out);
  TDN_LAUNCH_CHECK();
  return 0;
}

int roi_bwd(const char* who, const BalancedL1* bal, const void* cls, const void* reg, int dtype, int R, int C,
            int reg_cols, const int64_t* labels, const float* label_weights, const float* bbox_targets,
            const float* bbox_weights, float beta, const float* g, const float* avg_in, void* dcls, void* dreg,
            void* stream) {
  if (R == 0) return 0;
  TDN_CHECK(cls && reg && labels && label_weights && bbox_targets && bbox_weights && g && avg_in && dcls && dreg,
            "%s: NULL pointer", who);
  RoiArgs A;
  memset(&A, 0, sizeof(A));
  A.cls = cls;
  A.reg = reg;
  A.dcls = dcls;
  A.dreg = dreg;
  A.labels = labels;
  A.lw = label_weights;
  A.bt = bbox_targets;
  A.bw = bbox_weights;
  A.R = R;
  A.C = C;
  A.reg_cols = reg_cols;
  A.beta = beta;
  if (bal) A.bal = *bal;
  double* none = nullptr;
  if (bal) LOSS_LAUNCH_ROI(true, true, dtype, dim3(roi_blocks(R)), stream, A, g, avg_in, none);
  else LOSS_LAUNCH_ROI(true, false, dtype, dim3(roi_blocks(R)), stream, A, g, avg_in, none);
  TDN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int tdn_loss_roi_fwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                                const int64_t* labels, const float* label_weights, const float* bbox_targets,
                                const float* bbox_weights, float beta, const tdn_loss_avg* avg, float* losses,
                                float* avg_out, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_loss_roi_fwd";
  if (check_roi(who, dtype, R, C, reg_cols, beta) != 0) return -1;
  return roi_fwd(who, nullptr, cls, reg, dtype, R, C, reg_cols, labels, label_weights, bbox_targets, bbox_weights, beta,
                 avg, losses, avg_out, workspace, workspace_bytes, stream);
}

extern "C" int tdn_loss_roi_bwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                                const int64_t* labels, const float* label_weights, const float* bbox_targets,
                                const float* bbox_weights, float beta, const float* g, const float* avg_in, void* dcls,
                                void* dreg, void* stream) {
  const char* who = "tdn_loss_roi_bwd";
  if (check_roi(who, dtype, R, C, reg_cols, beta) != 0) return -1;
  return roi_bwd(who, nullptr, cls, reg, dtype, R, C, reg_cols, labels, label_weights, bbox_targets, bbox_weights, beta, g,
                 avg_in, dcls, dreg, stream);
}

extern "C" int tdn_loss_roi_balanced_fwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                                         const int64_t* labels, const float* label_weights, const float* bbox_targets,
                                         const float* bbox_weights, float beta, float alpha, float gamma,
                                         const tdn_loss_avg* avg, float* losses, float* avg_out, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_loss_roi_balanced_fwd";
  BalancedL1 P;
  if (check_roi(who, dtype, R, C, reg_cols, beta) != 0 || balanced_params(who, beta, alpha, gamma, &P) != 0) return -1;
  return roi_fwd(who, &P, cls, reg, dtype, R, C, reg_cols, labels, label_weights, bbox_targets, bbox_weights, beta, avg,
                 losses, avg_out, workspace, workspace_bytes, stream);
}

extern "C" int tdn_loss_roi_balanced_bwd(const void* cls, const void* reg, int dtype, int R, int C, int reg_cols,
                                         const int64_t* labels, const float* label_weights, const float* bbox_targets,
                                         const float* bbox_weights, float beta, float alpha, float gamma, const float* g,
                                         const float* avg_in, void* dcls, void* dreg, void* stream) {
  const char* who = "tdn_loss_roi_balanced_bwd";
  BalancedL1 P;
  if (check_roi(who, dtype, R, C, reg_cols, beta) != 0 || balanced_params(who, beta, alpha, gamma, &P) != 0) return -1;
  return roi_bwd(who, &P, cls, reg, dtype, R, C, reg_cols, labels, label_weights, bbox_targets, bbox_weights, beta, g,
                 avg_in, dcls, dreg, stream);
}
