// Gradient-harmonised losses of the dense anchor heads: GHM-C (classification) and GHM-R (regression) with their
// gradients (gfx950; DESIGN.md §4v has the spec, tests/ghm_ref.py restates it operation for operation).
//
// An element's weight is beta[row][bin]: the element's gradient norm g picks the bin, the row's histogram of g (smoothed
// over calls by the running average acc) gives beta.  Forward, four launches for all levels and both losses:
//   count     every workgroup counts its elements into an LDS histogram [kind][row][bin] (integer LDS adds) and stores it
//             to the workspace with plain stores;
//   table     one workgroup adds the workgroups' histograms (integers: no order), advances acc row after row and writes
//             the beta / tot table;
//   loss      beta * l per element, fp64 partial per (segment, workgroup);
//   final     partials in index order, per row / tot in fp64, rows in order, one rounding.
// Backward, one launch: g and the bin again, beta and tot from the forward's table; counts and acc are not touched.
// Per-element work is fp32 with explicit __f*_rn arithmetic (this file is compiled with -ffp-contract=off) and the
// soft_exp of soft_nms_core.h.  An element whose weight is not > 0 is never evaluated.  No float atomics, no host
// synchronisation, no allocation; every launch goes through TDN_LAUNCH.
#include "loss_core.h"
#include "soft_nms_core.h"
#include <string.h>

namespace {

constexpr int GT = 1024;            // threads per workgroup: 16 waves
constexpr int GWAVES = GT / 64;
constexpr int GMAX_BLOCKS = 256;    // one workgroup per CU at most
constexpr int MAXSEG = HEAD_MAXSEG;
constexpr int MAXROW = TDN_LOSS_MAX_LEVELS;
constexpr int NB = TDN_GHM_MAX_BINS;
constexpr int SB = NB + 1;          // histogram slots of a (kind, row): the bins, then "valid but in no bin" (NaN)
constexpr int NSLOT = 2 * MAXROW * SB;
constexpr int TS = TDN_GHM_TABLE_STRIDE;
constexpr int T_CNT = NB, T_TOT = 2 * NB, T_NR = 2 * NB + 1, T_NAN = 2 * NB + 2;
static_assert(TS >= T_NAN + 1, "a table row holds beta, the counts, tot, n and the NaN count");

enum { COUNT = 0, LOSS = 1, GRAD = 2 };

// ---- elementwise spec ------------------------------------------------------------------------------------------------
struct GhmVal {
  float g, l, dl;                   // gradient norm, element loss, d l / d x
};

// GHM-C: sigma by the sign of its argument (never sigma(x) - 1); a NaN logit stays NaN (soft_exp would turn it into -64)
__device__ __forceinline__ GhmVal ghm_cls(float x, bool t) {
  GhmVal v;
  if (x != x) {
    v.g = v.l = v.dl = x;
    return v;
  }
  const float e = soft_exp(-fabsf(x));
  const float den = __fadd_rn(1.f, e);
  const bool nonneg = t ? (-x >= 0.f) : (x >= 0.f);                  // sigma's argument: -x for a target, else x
  v.g = __fdiv_rn(nonneg ? 1.f : e, den);
  v.l = __fadd_rn(fmaxf(t ? -x : x, 0.f), log1pf(e));
  v.dl = t ? -v.g : v.g;
  return v;
}

// GHM-R: l = d^2 / (q + mu) is sqrt(d^2 + mu^2) - mu without the cancellation.  The square root is sqrtf, which hipcc
// rounds correctly (its default -fhip-fp32-correctly-rounded-divide-sqrt); this toolchain's __fsqrt_rn is the hardware's
// approximate instruction (it missed the rounded value by one ulp on the GPU), and the oracle's bits need the rounded one
__device__ __forceinline__ GhmVal ghm_reg(float x, float target, float mu, float mu2) {
  GhmVal v;
  const float d = __fsub_rn(x, target);
  const float dd = __fmul_rn(d, d);
  const float q = sqrtf(__fadd_rn(dd, mu2));
  v.g = __fdiv_rn(fabsf(d), q);
  v.l = __fdiv_rn(dd, __fadd_rn(q, mu));
  v.dl = __fdiv_rn(d, q);
  return v;
}

// the i with edge[i] <= g < edge[i + 1], the last bin closed above: the product guesses, the table decides (g is no NaN)
__device__ __forceinline__ int ghm_bin(float g, const float* edge, int bins) {
  int i = (int)__fmul_rn(g, (float)bins);
  i = min(max(i, 0), bins - 1);
  while (i > 0 && g < edge[i]) --i;
  while (i < bins - 1 && g >= edge[i + 1]) ++i;
  return i;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------
// The segments (one head tensor of one level each) and their walk in 16-byte chunks are loss_core.h's, shared with the
// dense loss kernel; here a workgroup walks segment after segment, 1024 consecutive chunks per grid
// stride, so that a segment's sum is a partial of its own.  HeadSeg::row: the level, or 0 with scope 'batch'.
typedef HeadSeg GhmSeg;
struct GhmArgs {
  GhmSeg seg[MAXSEG];
  int32_t nseg, rows;
  const int64_t* labels;
  const float* lw;
  const float* bt;
  const float* bw;
  int32_t N, A, C;
  int32_t bins[2];
  float mu, mu2;
  float edge[2][SB];   // edge[k][i] = fp32(i) / fp32(bins[k]), formed on the host; GHM-R's last edge is 1e3
};

struct GhmLds {
  float edge[2][SB];
  float beta[2 * MAXROW * NB];
  uint32_t hist[NSLOT];
  double red[2][GWAVES];
};

template <int DT, int MODE>
__device__ __forceinline__ double ghm_chunk(const GhmSeg& S, const GhmArgs& A, uint32_t lc, float scale, GhmLds& sh) {
  typedef Elem<DT> E;
  typedef typename E::T T;
  constexpr int V = E::V;
  const uint32_t m0 = lc * (uint32_t)V;
  const int cnt = (int)min((uint32_t)V, S.n - m0);
  const Vec<T, V> in = head_load<DT>(S, m0, cnt);
  Vec<T, V> out;
  const int bins = A.bins[S.reg];
  const float* edge = sh.edge[S.reg];
  const float* beta = sh.beta + (S.reg * MAXROW + S.row) * NB;
  uint32_t* hist = sh.hist + (S.reg * MAXROW + S.row) * SB;
  // coordinates of the chunk's first element; the following elements advance them
  const int div = S.reg ? 4 : A.C;               // channels per anchor
  HeadPos P = head_pos(S, m0, div);
  int last_idx = -1;
  bool last_valid = false;
  long long last_lab = 0;
  int run_slot = -1;                             // COUNT: equal slots in a row go to the histogram as one add
  uint32_t run = 0;
  double sum = 0.0;                              // the chunk's elements in memory order
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float res = 0.f;
    if (e < cnt) {
      const int idx = (int)P.b * A.N + S.off + (int)P.p * A.A + P.a;     // < 64 * 2^20
      const int k = P.k;
      const float x = E::ld(in.v[e]);
      bool valid;
      GhmVal v = {0.f, 0.f, 0.f};
      if (S.reg) {
        valid = A.bw[(size_t)idx * 4 + k] > 0.f;
        if (valid) v = ghm_reg(x, A.bt[(size_t)idx * 4 + k], A.mu, A.mu2);
      } else {
        if (idx != last_idx) {
          last_idx = idx;
          last_valid = A.lw[idx] > 0.f;
          if (last_valid) last_lab = A.labels[idx];
        }
        valid = last_valid;
        if (valid) v = ghm_cls(x, last_lab == (long long)k + 1);
      }
      if (valid) {
        int slot = NB;
        if (v.g == v.g) {
          slot = ghm_bin(v.g, edge, bins);
          if (MODE == LOSS) sum += (double)__fmul_rn(beta[slot], v.l);
          if (MODE == GRAD) res = __fmul_rn(__fmul_rn(beta[slot], v.dl), scale);
        } else {                                 // in no bin: the NaN goes on, for the optimizer's overflow check
          if (MODE == LOSS) sum += (double)v.g;
          if (MODE == GRAD) res = v.g;
        }
        if (MODE == COUNT) {
          if (slot != run_slot) {
            if (run) atomicAdd(&hist[run_slot], run);
            run_slot = slot;
            run = 0;
          }
          ++run;
        }
      }
      head_next(S, div, P);
    }
    if (MODE == GRAD) out.v[e] = E::st(res);
  }
  if (MODE == COUNT && run) atomicAdd(&hist[run_slot], run);
  if (MODE == GRAD) head_store<DT>(S, m0, cnt, out);
  return sum;
}

// COUNT: counts [gridDim.x][NSLOT]; LOSS: partials [nseg][gridDim.x]; GRAD: the segments' dx.  table: the forward's
// (LOSS, GRAD); g: the cotangent (GRAD)
template <int DT, int MODE>
__global__ __launch_bounds__(GT) void ghm_walk_kernel(const GhmArgs A, const float* __restrict__ g,
                                                      const float* __restrict__ table, uint32_t* __restrict__ counts,
                                                      double* __restrict__ partials) {
  __shared__ GhmLds sh;
  const int t = threadIdx.x;
  if (t == 0) {
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < SB; ++i) sh.edge[k][i] = A.edge[k][i];     // uniform indices: scalar loads of the arguments
  }
  if (MODE == COUNT) {
    for (int i = t; i < NSLOT; i += GT) sh.hist[i] = 0u;
  } else {
    for (int i = t; i < 2 * MAXROW * NB; i += GT) sh.beta[i] = table[(i / NB) * TS + (i % NB)];
  }
  __syncthreads();
  for (int s = 0; s < A.nseg; ++s) {                       // s is uniform: the segment comes through scalar loads
    const GhmSeg& S = A.seg[s];
    float scale = 0.f;
    if (MODE == GRAD) scale = __fdiv_rn(g[S.reg], table[(S.reg * MAXROW + S.row) * TS + T_TOT]);
    double acc = 0.0;
    for (uint32_t c0 = blockIdx.x * (uint32_t)GT; c0 < S.nchunks; c0 += gridDim.x * (uint32_t)GT) {
      const uint32_t lc = c0 + (uint32_t)t;
      if (lc < S.nchunks) acc += ghm_chunk<DT, MODE>(S, A, lc, scale, sh);
    }
    if (MODE == LOSS) {
      // lanes -> xor tree, waves -> wave 0 .. 15 in order.  red is double-buffered: buffer s & 1 is written again for
      // segment s + 2, which a wave reaches only through the barrier of segment s + 1, after thread 0 has read it
      acc = wave_sum(acc);
      if ((t & 63) == 0) sh.red[s & 1][t >> 6] = acc;
      __syncthreads();
      if (t == 0) {
        double v = 0.0;
        for (int w = 0; w < GWAVES; ++w) v += sh.red[s & 1][w];
        partials[(size_t)s * gridDim.x + blockIdx.x] = v;
      }
    }
  }
  if (MODE == COUNT) {
    __syncthreads();
    for (int i = t; i < NSLOT; i += GT) counts[(size_t)blockIdx.x * NSLOT + i] = sh.hist[i];
  }
}

// ---- the table: totals, the running average, beta ------------------------------------------------------------------------
struct TableArgs {
  int32_t rows, blocks;
  int32_t bins[2];
  float mmt[2];
};

// one workgroup.  acc_k fp32 [bins_k] (NULL with momentum 0) is advanced row after row, bin i by thread i; table fp32
// [2][MAXROW][TS] is written in full; tot64 [2][MAXROW] is what the last launch divides by
__global__ __launch_bounds__(GT) void ghm_table_kernel(const uint32_t* __restrict__ counts, const TableArgs P,
                                                       float* __restrict__ acc_cls, float* __restrict__ acc_reg,
                                                       float* __restrict__ table, double* __restrict__ tot64) {
  __shared__ unsigned long long cnt[NSLOT];
  __shared__ unsigned long long tot[2 * MAXROW];
  __shared__ int nr[2 * MAXROW];
  const int t = threadIdx.x;
  for (int i = t; i < NSLOT; i += GT) {
    unsigned long long s = 0ull;
    for (int b = 0; b < P.blocks; ++b) s += counts[(size_t)b * NSLOT + i];
    cnt[i] = s;
  }
  __syncthreads();
  if (t < 2 * MAXROW) {                                    // (kind, row) = t
    const int kind = t / MAXROW, r = t % MAXROW;
    const unsigned long long* c = cnt + t * SB;
    unsigned long long n = 0ull;
    int ne = 0;
    if (r < P.rows) {
      n = c[NB];
      for (int i = 0; i < P.bins[kind]; ++i) {
        n += c[i];
        ne += c[i] != 0ull;
      }
    }
    n = n < 1ull ? 1ull : n;
    tot[t] = n;
    nr[t] = ne;
    tot64[t] = (double)n;
    float* T = table + t * TS;
    T[T_TOT] = (float)n;
    T[T_NR] = (float)ne;
    T[T_NAN] = r < P.rows ? (float)c[NB] : 0.f;
    for (int j = T_NAN + 1; j < TS; ++j) T[j] = 0.f;
  }
  __syncthreads();
  if (t < 2 * NB) {                                        // (kind, bin) = t: a bin's running average is its own chain
    const int kind = t / NB, i = t % NB;
    const bool live = i < P.bins[kind];
    const float mmt = P.mmt[kind];
    const float omm = __fsub_rn(1.f, mmt);
    float* acc = kind ? acc_reg : acc_cls;
    float a = (live && mmt > 0.f) ? acc[i] : 0.f;
    for (int r = 0; r < MAXROW; ++r) {
      const int kr = kind * MAXROW + r;
      float beta = 0.f, fc = 0.f;
      if (live && r < P.rows) {
        const unsigned long long c = cnt[kr * SB + i];
        fc = (float)c;
        if (c != 0ull) {
          const float ftot = (float)tot[kr];
          float w;
          if (mmt > 0.f) {
            a = __fadd_rn(__fmul_rn(mmt, a), __fmul_rn(omm, fc));
            w = __fdiv_rn(ftot, a);
          } else {
            w = __fdiv_rn(ftot, fc);
          }
          beta = __fdiv_rn(w, (float)nr[kr]);
        }
      }
      table[kr * TS + i] = beta;
      table[kr * TS + T_CNT + i] = fc;
    }
    if (live && mmt > 0.f) acc[i] = a;
  }
}

// ---- last launch: partials in index order, per row / tot, rows in order, one rounding -----------------------------------
// segment s = 2 * level + kind; its row is the level, or 0 with scope 'batch'
__global__ __launch_bounds__(64) void ghm_final_kernel(const double* __restrict__ partials, int blocks, int nseg,
                                                       int batch_scope, const double* __restrict__ tot64,
                                                       float* __restrict__ losses) {
  __shared__ double segsum[MAXSEG];
  const int t = threadIdx.x;
  if (t < nseg) {
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partials[(size_t)t * blocks + b];
    segsum[t] = s;
  }
  __syncthreads();
  if (t < 2) {                                             // kind = t
    double total = 0.0;
    if (batch_scope) {
      double rs = 0.0;
      for (int s = t; s < nseg; s += 2) rs += segsum[s];
      total = rs / tot64[t * MAXROW];
    } else {
      for (int s = t; s < nseg; s += 2) total += segsum[s] / tot64[t * MAXROW + (s >> 1)];
    }
    losses[t] = (float)total;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct GhmWs {
  uint32_t* counts;
  double* partials;
  double* tot64;
  int64_t bytes;
};
GhmWs ghm_layout(int blocks, void* base) {     // a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<uint32_t>((int64_t)blocks * NSLOT), c.take<double>((int64_t)blocks * MAXSEG),
          c.take<double>(2 * MAXROW), c.off};
}

// The shape half of the plan, all the size query needs: the limits of §4e with those of the GHM configuration, the
// segment table without its pointers.  Returns the number of workgroups, or -1 with the error set.
int ghm_shape(const char* who, const tdn_loss_level* levels, int L, int B, const tdn_ghm_config* cfg, GhmArgs* D) {
  TDN_CHECK(levels && cfg, "%s: NULL argument", who);
  TDN_CHECK(L >= 1 && L <= TDN_LOSS_MAX_LEVELS, "%s: %d levels (1..%d)", who, L, TDN_LOSS_MAX_LEVELS);
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(cfg->dtype == TDN_F32 || cfg->dtype == TDN_BF16 || cfg->dtype == TDN_F16, "%s: dtype %d", who, cfg->dtype);
  TDN_CHECK(cfg->num_anchors >= 1 && cfg->num_classes >= 1 && cfg->num_classes <= TDN_LOSS_MAX_CLASSES,
            "%s: A=%d, C=%d (C in 1..%d)", who, cfg->num_anchors, cfg->num_classes, TDN_LOSS_MAX_CLASSES);
  TDN_CHECK(cfg->bins_cls >= 1 && cfg->bins_cls <= NB && cfg->bins_reg >= 1 && cfg->bins_reg <= NB,
            "%s: bins_cls=%d, bins_reg=%d (1..%d each)", who, cfg->bins_cls, cfg->bins_reg, NB);
  TDN_CHECK(cfg->momentum_cls >= 0.f && cfg->momentum_cls < 1.f && cfg->momentum_reg >= 0.f && cfg->momentum_reg < 1.f,
            "%s: momentum_cls=%g, momentum_reg=%g (each in [0, 1))", who, (double)cfg->momentum_cls,
            (double)cfg->momentum_reg);
  TDN_CHECK(cfg->mu > 0.f && cfg->mu < INFINITY, "%s: mu must be finite and > 0", who);
  TDN_CHECK(cfg->scope == TDN_GHM_SCOPE_LEVEL || cfg->scope == TDN_GHM_SCOPE_BATCH, "%s: scope %d is neither level (0) "
            "nor batch (1)", who, cfg->scope);
  memset(D, 0, sizeof(*D));
  const int A = cfg->num_anchors, C = cfg->num_classes;
  int64_t chunks = 0, most = 1;
  const int64_t N = head_segments(who, levels, L, B, cfg->dtype, A, C, D->seg, &chunks);
  if (N < 0) return -1;
  for (int s = 0; s < 2 * L; ++s) {
    GhmSeg& S = D->seg[s];
    S.row = cfg->scope == TDN_GHM_SCOPE_BATCH ? 0 : s / 2;
    most = S.nchunks > most ? S.nchunks : most;
  }
  D->nseg = 2 * L;
  D->rows = cfg->scope == TDN_GHM_SCOPE_BATCH ? 1 : L;
  D->N = (int32_t)N;
  D->A = A;
  D->C = C;
  D->bins[0] = cfg->bins_cls;
  D->bins[1] = cfg->bins_reg;
  D->mu = cfg->mu;
  D->mu2 = (float)((double)cfg->mu * (double)cfg->mu);
  for (int k = 0; k < 2; ++k) {
    for (int i = 0; i <= D->bins[k]; ++i) D->edge[k][i] = (float)i / (float)D->bins[k];
  }
  D->edge[1][D->bins[1]] = 1000.f;             // mmdetection's last GHM-R edge: g <= 1 lies in the last bin
  const int64_t blocks = (most + GT - 1) / GT;
  return (int)(blocks < GMAX_BLOCKS ? blocks : GMAX_BLOCKS);
}

// The pointer half: each segment's tensors and the targets.  Same return value.
int ghm_plan(const char* who, const tdn_loss_level* levels, int L, int B, const tdn_ghm_config* cfg,
             const int64_t* labels, const float* lw, const float* bt, const float* bw, bool grad, GhmArgs* D) {
  const int blocks = ghm_shape(who, levels, L, B, cfg, D);
  if (blocks < 0) return -1;
  TDN_CHECK(labels && lw && bt && bw, "%s: NULL pointer", who);
  if (head_pointers(who, levels, L, grad, D->seg) != 0) return -1;
  D->labels = labels;
  D->lw = lw;
  D->bt = bt;
  D->bw = bw;
  return blocks;
}

#define GHM_LAUNCH_DT(MODE, dtype, grid, st, ...)                                                              \
  do {                                                                                                         \
    if ((dtype) == TDN_F32) TDN_LAUNCH((ghm_walk_kernel<TDN_F32, MODE>), grid, dim3(GT), 0, st, __VA_ARGS__);   \
    else if ((dtype) == TDN_F16) TDN_LAUNCH((ghm_walk_kernel<TDN_F16, MODE>), grid, dim3(GT), 0, st, __VA_ARGS__); \
    else TDN_LAUNCH((ghm_walk_kernel<TDN_BF16, MODE>), grid, dim3(GT), 0, st, __VA_ARGS__);                     \
  } while (0)

}  // namespace

extern "C" int64_t tdn_ghm_workspace_bytes(const tdn_loss_level* levels, int num_levels, int B,
                                           const tdn_ghm_config* cfg) {
  GhmArgs D;
  const int blocks = ghm_shape("tdn_ghm_workspace_bytes", levels, num_levels, B, cfg, &D);
  return blocks < 0 ? -1 : ghm_layout(blocks, nullptr).bytes;
}

extern "C" int tdn_ghm_fwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_ghm_config* cfg,
                           const int64_t* labels, const float* label_weights, const float* bbox_targets,
                           const float* bbox_weights, float* acc_cls, float* acc_reg, float* losses, float* table,
                           void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_ghm_fwd";
  GhmArgs D;
  const int blocks = ghm_plan(who, levels, num_levels, B, cfg, labels, label_weights, bbox_targets, bbox_weights, false,
                              &D);
  if (blocks < 0) return -1;
  TDN_CHECK(losses && table && workspace, "%s: NULL pointer", who);
  TDN_CHECK((cfg->momentum_cls == 0.f || acc_cls) && (cfg->momentum_reg == 0.f || acc_reg),
            "%s: momentum > 0 needs its acc tensor", who);
  const GhmWs w = ghm_layout(blocks, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  const float* nof = nullptr;
  double* nod = nullptr;
  uint32_t* nou = nullptr;
  GHM_LAUNCH_DT(COUNT, cfg->dtype, dim3(blocks), stream, D, nof, nof, w.counts, nod);
  TDN_LAUNCH_CHECK();
  const TableArgs P = {D.rows, blocks, {D.bins[0], D.bins[1]}, {cfg->momentum_cls, cfg->momentum_reg}};
  TDN_LAUNCH(ghm_table_kernel, dim3(1), dim3(GT), 0, stream, (const uint32_t*)w.counts, P, acc_cls, acc_reg, table,
             w.tot64);
  TDN_LAUNCH_CHECK();
  GHM_LAUNCH_DT(LOSS, cfg->dtype, dim3(blocks), stream, D, nof, (const float*)table, nou, w.partials);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(ghm_final_kernel, dim3(1), dim3(64), 0, stream, (const double*)w.partials, blocks, D.nseg,
             cfg->scope == TDN_GHM_SCOPE_BATCH ? 1 : 0, (const double*)w.tot64, losses);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_ghm_bwd(const tdn_loss_level* levels, int num_levels, int B, const tdn_ghm_config* cfg,
                           const int64_t* labels, const float* label_weights, const float* bbox_targets,
                           const float* bbox_weights, const float* g, const float* table, void* stream) {
  const char* who = "tdn_ghm_bwd";
  GhmArgs D;
  const int blocks = ghm_plan(who, levels, num_levels, B, cfg, labels, label_weights, bbox_targets, bbox_weights, true,
                              &D);
  if (blocks < 0) return -1;
  TDN_CHECK(g && table, "%s: NULL pointer", who);
  double* nod = nullptr;
  uint32_t* nou = nullptr;
  GHM_LAUNCH_DT(GRAD, cfg->dtype, dim3(blocks), stream, D, g, table, nou, nod);
  TDN_LAUNCH_CHECK();
  return 0;
}
