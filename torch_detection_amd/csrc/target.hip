// Training targets: max-IoU assignment, random sampling, RPN (anchor_target) and RoI-head (sample_rois) targets
// (DESIGN.md §4d).
//
// Semantics are the project's own spec in the mmdetection-v0.x/v1 lineage (MaxIoUAssigner, RandomSampler, anchor_target,
// bbox_target) on '+1' boxes; the IoU is box.hip's (nms_core.h) and the encode §4b's (delta_core.h), strict IEEE fp32:
// this file is compiled with -ffp-contract=off.  The CPU restatement is tests/target_ref.py.
//
// The (N, G) IoU matrix never reaches memory.  A call is
//   0 target_clear_kernel     column maxima <- 0, first indices <- INT_MAX (the only workspace words read before written)
//   1 assign_pass1_kernel     one lane per box, the image's ground truths in LDS: row maximum / argmax -> the step-4/5
//                             label and max_overlaps; column maxima as IoU bit patterns (IoU >= 0: they order like the
//                             values): LDS atomicMax inside the workgroup, then one global atomicMax per ground truth
//                             and workgroup that can still raise it
//   2 assign_pass2_kernel     the same IoUs again (same instructions, same bits) against the column maxima: step 6, or
//                             with gt_max_assign_all = 0 the lowest box attaining each maximum (integer atomicMin)
//  2b assign_first_kernel     gt_max_assign_all = 0 only: those boxes get their highest such ground truth
//   3 sample_select_kernel    two workgroups per image (positives, negatives): class counts, radix select of the k-th
//                             smallest (key, index) (select_core.h), masks written in index order
//   4 anchor_target_fill_kernel / sample_rois_fill_kernel   encode and every output fill
// Integer atomics only (maximum, minimum, counts): every output is a pure function of the inputs.
#include "nms_core.h"
#include "select_core.h"
#include "delta_core.h"
#include <limits.h>
#include <string.h>

constexpr int MAXG = TDN_TARGET_MAX_GT;
constexpr int P1_THREADS = 256;
constexpr int P1_PER = 4;                      // boxes per thread: 1024 per workgroup share one LDS copy of the gts

// Where box i of image b comes from, and whether it takes part.
struct BoxSrc {
  const float* boxes;          // anchor mode: [N][4] (stride 0) or [B][N][4]
  int64_t stride;
  const uint8_t* valid;        // [N] (vstride 0) or [B][N] (vstride N), or NULL; independent of `stride`
  int64_t vstride;
  const int32_t* img_shapes;   // with border >= 0: [B][2] = (h, w)
  int border;
  int cand;                    // candidate mode: the image's ground truths (add_gt), then its counts[b] proposals
  const float* props;          // [B][P][5]
  const int32_t* counts;       // [B]
  int P, add_gt;
  const float* gt;             // [B][G][4]
  int G;
};

__device__ __forceinline__ bool fetch_box(const BoxSrc& S, int b, int i, int Gb, f32x4_t* out) {
  if (S.cand) {
    const int ng = S.add_gt ? Gb : 0;
    if (i < ng) {
      *out = *(const f32x4_t*)(S.gt + ((int64_t)b * S.G + i) * 4);
      return true;
    }
    const int p = i - ng;
    const int cnt = min(max(S.counts[b], 0), S.P);
    if (p >= cnt) return false;
    const float* r = S.props + ((int64_t)b * S.P + p) * 5;
    *out = (f32x4_t){r[0], r[1], r[2], r[3]};
    return true;
  }
  if (S.valid && S.valid[b * S.vstride + i] == 0) return false;
  const f32x4_t bx = *(const f32x4_t*)(S.boxes + b * S.stride + (int64_t)i * 4);
  *out = bx;
  if (S.border >= 0) {
    const float lo = (float)(-S.border);
    const float hy = (float)(S.img_shapes[2 * b] + S.border), hx = (float)(S.img_shapes[2 * b + 1] + S.border);
    return bx[0] >= lo && bx[1] >= lo && bx[2] < hx && bx[3] < hy;
  }
  return true;
}

struct AssignArgs {
  BoxSrc S;
  const int32_t* gt_counts;
  int N, G, all;
  float pos_thr, neg_thr, min_pos;
};

__device__ __forceinline__ int gt_count(const int32_t* gt_counts, int b, int G) {
  return min(max(gt_counts[b], 0), G);
}

__global__ void target_clear_kernel(uint32_t* colmax, int* first, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    colmax[i] = 0u;
    first[i] = INT_MAX;
  }
}

__global__ __launch_bounds__(P1_THREADS) void assign_pass1_kernel(const AssignArgs A, int32_t* __restrict__ assigned,
                                                                  float* __restrict__ max_overlaps, uint32_t* colmax) {
  __shared__ f32x4_t sgt[MAXG];
  __shared__ float sarea[MAXG];
  __shared__ uint32_t scol[MAXG];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int Gb = gt_count(A.gt_counts, b, A.G);
  for (int j = tid; j < Gb; j += P1_THREADS) {
    const f32x4_t g = *(const f32x4_t*)(A.S.gt + ((int64_t)b * A.G + j) * 4);
    sgt[j] = g;
    sarea[j] = box_area(g);
    scol[j] = 0u;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < P1_PER; ++k) {
    const int i = (blockIdx.x * P1_PER + k) * P1_THREADS + tid;
    if (i >= A.N) break;
    f32x4_t bx;
    const bool ok = fetch_box(A.S, b, i, Gb, &bx);
    int a = -1;
    float mx = 0.f;
    if (ok) {
      if (Gb == 0) {
        a = 0;
      } else {
        const float area = box_area(bx);
        int am = 0;
        mx = -1.f;
        for (int j = 0; j < Gb; ++j) {
          const float v = box_iou2(bx, area, sgt[j], sarea[j]);      // LDS broadcast reads
          if (v > mx) {
            mx = v;
            am = j;
          }
          const uint32_t bits = __float_as_uint(v);
          if (v > 0.f && bits > scol[j]) atomicMax(&scol[j], bits);
        }
        if (mx >= 0.f && mx < A.neg_thr) a = 0;
        if (mx >= A.pos_thr) a = am + 1;
        if (!(mx >= 0.f)) mx = 0.f;
      }
    }
    assigned[(int64_t)b * A.N + i] = a;
    if (max_overlaps) max_overlaps[(int64_t)b * A.N + i] = mx;
  }
  __syncthreads();
  for (int j = tid; j < Gb; j += P1_THREADS) {
    const uint32_t v = scol[j];
    uint32_t* g = colmax + b * A.G + j;
    if (v != 0u && v > *(volatile uint32_t*)g) atomicMax(g, v);     // a stale read only costs a redundant atomic
  }
}

__global__ __launch_bounds__(P1_THREADS) void assign_pass2_kernel(const AssignArgs A, int32_t* __restrict__ assigned,
                                                                  const uint32_t* __restrict__ colmax, int* first) {
  __shared__ f32x4_t sgt[MAXG];
  __shared__ float sarea[MAXG];
  __shared__ float sgm[MAXG];                  // the column maximum, or -1 where it is below min_pos_iou
  __shared__ int sfirst[MAXG];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int Gb = gt_count(A.gt_counts, b, A.G);
  if (Gb == 0) return;
  for (int j = tid; j < Gb; j += P1_THREADS) {
    const f32x4_t g = *(const f32x4_t*)(A.S.gt + ((int64_t)b * A.G + j) * 4);
    sgt[j] = g;
    sarea[j] = box_area(g);
    const float gm = __uint_as_float(colmax[b * A.G + j]);
    sgm[j] = gm >= A.min_pos ? gm : -1.f;
    sfirst[j] = INT_MAX;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < P1_PER; ++k) {
    const int i = (blockIdx.x * P1_PER + k) * P1_THREADS + tid;
    if (i >= A.N) break;
    f32x4_t bx;
    if (!fetch_box(A.S, b, i, Gb, &bx)) continue;
    const float area = box_area(bx);
    int a = -1;
    for (int j = 0; j < Gb; ++j) {
      const float v = box_iou2(bx, area, sgt[j], sarea[j]);
      if (v == sgm[j]) {
        a = j + 1;                             // the highest such j stays
        if (!A.all) atomicMin(&sfirst[j], i);
      }
    }
    if (A.all && a > 0) assigned[(int64_t)b * A.N + i] = a;
  }
  if (A.all) return;
  __syncthreads();
  for (int j = tid; j < Gb; j += P1_THREADS)
    if (sfirst[j] != INT_MAX) atomicMin(first + b * A.G + j, sfirst[j]);
}

// gt_max_assign_all = 0: box first[j] gets j + 1; where several j name one box, the highest wins
__global__ __launch_bounds__(MAXG) void assign_first_kernel(const int* __restrict__ first, const int32_t* gt_counts,
                                                            int N, int G, int32_t* assigned) {
  __shared__ int sf[MAXG];
  const int j = threadIdx.x, b = blockIdx.x;
  const int Gb = gt_count(gt_counts, b, G);
  const int mine = j < Gb ? first[b * G + j] : INT_MAX;
  sf[j] = mine;
  __syncthreads();
  if (mine == INT_MAX) return;
  for (int h = j + 1; h < Gb; ++h)
    if (sf[h] == mine) return;
  assigned[(int64_t)b * N + mine] = j + 1;
}

// ---- sampling ---------------------------------------------------------------------------------------------------
// The generated key of box i of image b: lowbias32 of the three words mixed by odd multipliers, top 31 bits.
__host__ __device__ __forceinline__ uint32_t target_key(uint32_t seed, uint32_t b, uint32_t i) {
  uint32_t h = seed ^ (b * 0x9E3779B9u) ^ (i * 0x85EBCA6Bu);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h >> 1;
}

// Selection keys of one class of one image: members get 0x80000000 | (0x7FFFFFFF - key), so the k HIGHEST with ties to
// the lower index are the k smallest (key, index); everything else is 0, below every member.
struct ClassFetch {
  const int32_t* assigned;     // the image's row
  const int32_t* keys;         // the image's row, or NULL
  uint32_t seed, b;
  int cls;                     // 0: assigned > 0, 1: assigned == 0
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (e < cnt) {
        const int a = assigned[i0 + e];
        const bool member = cls ? a == 0 : a > 0;
        const uint32_t key = keys ? ((uint32_t)keys[i0 + e] & 0x7FFFFFFFu) : target_key(seed, b, (uint32_t)(i0 + e));
        kk[e] = member ? (0x80000000u | (0x7FFFFFFFu - key)) : 0u;
      }
  }
};

// The marking pass of a selection: key > T is taken, key == T while fewer than `need` of them came before in index order.
// CLEAR: a byte that is not taken becomes 0 (the row is this selection's alone); else it keeps what it holds (the row
// collects several selections).
template <bool CLEAR, class Fetch>
__device__ __forceinline__ void mark_selected(const Fetch& F, int N, uint32_t T, int need, uint8_t* mrow, int* misc) {
  const int tid = threadIdx.x;
  int ties_done = 0;
  for (int base = 0; base < N; base += TK_STEP) {
    const int i0 = base + tid * TK_PER;
    const int cnt = max(0, min(TK_PER, N - i0));
    uint32_t kk[TK_PER];
    if (cnt > 0) F(i0, cnt, kk);
    int tpos = 0;
    if (need > 0) {                            // workgroup-uniform
      int nt = 0, tot;
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) nt += kk[e] == T ? 1 : 0;
      tpos = ties_done + block_excl_scan(nt, misc, &tot);
      ties_done += tot;
    }
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (e < cnt) {
        bool sel = kk[e] > T;
        if (kk[e] == T) {
          sel = tpos < need;
          ++tpos;
        }
        if (CLEAR) mrow[i0 + e] = sel ? 1 : 0;
        else if (sel) mrow[i0 + e] = 1;
      }
  }
}

// The k smallest (key, index) of the `members` of a class into mrow; k <= members.
__device__ __forceinline__ void select_class(const ClassFetch& F, int N, int k, int members, uint8_t* mrow, int* hist,
                                             int* misc) {
  uint32_t T;
  int need = 0;
  if (k == members) T = 0x7FFFFFFFu;           // every member
  else if (k == 0) T = 0xFFFFFFFFu;            // nothing
  else T = block_radix_threshold(F, N, k, hist, misc, &need);
  mark_selected<true>(F, N, T, need, mrow, misc);
}

struct SampleArgs {
  int N, num, num_pos_expected;
  double neg_pos_ub;
  uint32_t seed;
};

__global__ __launch_bounds__(1024) void sample_select_kernel(const SampleArgs A, const int32_t* __restrict__ assigned,
                                                             const int32_t* __restrict__ keys, uint8_t* pos_mask,
                                                             uint8_t* neg_mask, int32_t* num_pos, int32_t* num_neg) {
  __shared__ int hist[TK_BINS];
  __shared__ int misc[TK_MISC];
  const int tid = threadIdx.x, cls = blockIdx.x, b = blockIdx.y, N = A.N;
  const int32_t* arow = assigned + (int64_t)b * N;
  if (tid < 2) misc[32 + tid] = 0;
  __syncthreads();
  int cp = 0, cn = 0;
  for (int i = tid; i < N; i += BLK) {
    const int a = arow[i];
    cp += a > 0 ? 1 : 0;
    cn += a == 0 ? 1 : 0;
  }
  if (cp) atomicAdd(&misc[32], cp);
  if (cn) atomicAdd(&misc[33], cn);
  __syncthreads();
  const int npos = misc[32], nneg = misc[33];
  const int pos = min(npos, A.num_pos_expected);
  int neg_exp = A.num - pos;
  if (A.neg_pos_ub >= 0.0) {
    const double ub = A.neg_pos_ub * (double)max(1, pos);
    if (ub < (double)neg_exp) neg_exp = (int)ub;
  }
  const int neg = min(nneg, max(neg_exp, 0));
  const int k = cls ? neg : pos, members = cls ? nneg : npos;
  const ClassFetch F{arow, keys ? keys + (int64_t)b * N : nullptr, A.seed, (uint32_t)b, cls};
  select_class(F, N, k, members, (cls ? neg_mask : pos_mask) + (int64_t)b * N, hist, misc);
  if (tid == 0) (cls ? num_neg : num_pos)[b] = k;
}

// ---- IoU-balanced negatives (Libra R-CNN) -------------------------------------------------------------
// The positives are sample_select_kernel's.  The negatives of an image are chosen by a sequence of dependent keyed
// selections — "the k smallest (key, index) of a set" with the set changing from one to the next — run one after the
// other by the image's second workgroup; the byte row of neg_mask is the "taken" state between them.
struct BalancedArgs {
  float floor_thr, floor_fraction;
  int num_bins;
};

// negatives not taken yet, of one category: 0 a bin [lo, hi) of S, 1 S, 2 F (the floor set), 3 any
struct BalancedFetch {
  const int32_t* assigned;
  const float* ov;
  const int32_t* keys;
  const uint8_t* taken;
  uint32_t seed, b;
  int kind;
  float lo, hi, floor_thr;
  __device__ __forceinline__ bool in_s(float o) const {
    return floor_thr > 0.f ? o >= floor_thr : (floor_thr == 0.f ? o > 0.f : true);
  }
  __device__ __forceinline__ bool member(int i) const {
    if (assigned[i] != 0 || taken[i] != 0) return false;
    const float o = ov[i];
    if (kind == 0) return in_s(o) && o >= lo && o < hi;
    if (kind == 1) return in_s(o);
    if (kind == 2) return !in_s(o);          // the negatives outside S: 0 <= o < floor_thr, or o == 0 at floor_thr == 0
    return true;
  }
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (e < cnt) {
        const uint32_t key = keys ? ((uint32_t)keys[i0 + e] & 0x7FFFFFFFu) : target_key(seed, b, (uint32_t)(i0 + e));
        kk[e] = member(i0 + e) ? (0x80000000u | (0x7FFFFFFFu - key)) : 0u;
      }
  }
};

__device__ __forceinline__ int balanced_count(const BalancedFetch& F, int N, int* misc) {
  int c = 0, tot;
  for (int i = threadIdx.x; i < N; i += BLK) c += F.member(i) ? 1 : 0;
  block_excl_scan(c, misc, &tot);
  return tot;
}

// marks the k smallest (key, index) of F's members in mrow (all of them when there are no more than k); returns how many
__device__ __forceinline__ int balanced_take(const BalancedFetch& F, int N, int k, uint8_t* mrow, int* hist, int* misc) {
  const int members = balanced_count(F, N, misc);
  if (k <= 0 || members == 0) return 0;        // workgroup-uniform
  uint32_t T;
  int need = 0;
  if (k >= members) T = 0x7FFFFFFFu;
  else T = block_radix_threshold(F, N, k, hist, misc, &need);
  mark_selected<false>(F, N, T, need, mrow, misc);
  __syncthreads();                             // the marks are the next selection's "taken"
  return k < members ? k : members;
}

__global__ __launch_bounds__(1024) void sample_select_balanced_kernel(const SampleArgs A, const BalancedArgs Q,
                                                                      const int32_t* __restrict__ assigned,
                                                                      const float* __restrict__ overlaps,
                                                                      const int32_t* __restrict__ keys, uint8_t* pos_mask,
                                                                      uint8_t* neg_mask, int32_t* num_pos,
                                                                      int32_t* num_neg) {
  __shared__ int hist[TK_BINS];
  __shared__ int misc[TK_MISC];
  const int tid = threadIdx.x, cls = blockIdx.x, b = blockIdx.y, N = A.N;
  const int32_t* arow = assigned + (int64_t)b * N;
  const float* orow = overlaps + (int64_t)b * N;
  uint8_t* mrow = (cls ? neg_mask : pos_mask) + (int64_t)b * N;
  if (tid < 3) misc[32 + tid] = 0;
  __syncthreads();
  int cp = 0, cn = 0, om = 0;
  for (int i = tid; i < N; i += BLK) {
    const int a = arow[i];
    cp += a > 0 ? 1 : 0;
    cn += a == 0 ? 1 : 0;
    const float o = orow[i];
    if (o > 0.f) om = max(om, __float_as_int(o));          // positive floats order as their bit patterns
    if (cls) mrow[i] = 0;
  }
  if (cp) atomicAdd(&misc[32], cp);
  if (cn) atomicAdd(&misc[33], cn);
  if (om) atomicMax(&misc[34], om);
  __syncthreads();
  const int npos = misc[32], nneg = misc[33];
  const float m = __int_as_float(misc[34]);
  const int pos = min(npos, A.num_pos_expected);
  int neg_exp = A.num - pos;
  if (A.neg_pos_ub >= 0.0) {
    const double ub = A.neg_pos_ub * (double)max(1, pos);
    if (ub < (double)neg_exp) neg_exp = (int)ub;
  }
  const int n = max(neg_exp, 0);
  const int32_t* krow = keys ? keys + (int64_t)b * N : nullptr;
  if (cls == 0) {                              // the positives: sample_select_kernel's own code
    select_class(ClassFetch{arow, krow, A.seed, (uint32_t)b, 0}, N, pos, npos, mrow, hist, misc);
    if (tid == 0) num_pos[b] = pos;
    return;
  }
  BalancedFetch F{arow, orow, krow, mrow, A.seed, (uint32_t)b, 3, 0.f, 0.f, Q.floor_thr};
  if (nneg <= n) {                             // every negative
    balanced_take(F, N, nneg, mrow, hist, misc);
    if (tid == 0) num_neg[b] = nneg;
    return;
  }
  F.kind = 1;
  const int in_s = balanced_count(F, N, misc);
  const int n_s = (int)((double)n * (1.0 - (double)Q.floor_fraction));
  int got = 0;
  if (in_s <= n_s) {
    got = balanced_take(F, N, in_s, mrow, hist, misc);
  } else if (Q.num_bins >= 2) {
    const float t0 = Q.floor_thr > 0.f ? Q.floor_thr : 0.f;
    const float w = __fdiv_rn(__fsub_rn(m, t0), (float)Q.num_bins);
    const int per = n_s / Q.num_bins;
    F.kind = 0;
    for (int k = 0; k < Q.num_bins; ++k) {
      F.lo = __fadd_rn(t0, __fmul_rn((float)k, w));
      F.hi = __fadd_rn(t0, __fmul_rn((float)(k + 1), w));
      got += balanced_take(F, N, per, mrow, hist, misc);
    }
    F.kind = 1;
    if (got < n_s) got += balanced_take(F, N, n_s - got, mrow, hist, misc);
  } else {
    got = balanced_take(F, N, n_s, mrow, hist, misc);
  }
  F.kind = 2;
  got += balanced_take(F, N, n - got, mrow, hist, misc);
  F.kind = 3;
  if (got < n) balanced_take(F, N, n - got, mrow, hist, misc);
  if (tid == 0) num_neg[b] = n;
}

// ---- output fills -----------------------------------------------------------------------------------------------
struct FillArgs {
  BoxSrc S;
  const int32_t* gt_counts;
  int B, N, G, num;
  f32x4_t means, stds;
};

__global__ __launch_bounds__(256) void anchor_target_fill_kernel(const FillArgs A, const int32_t* __restrict__ assigned,
                                                                 const uint8_t* __restrict__ pos_mask,
                                                                 const uint8_t* __restrict__ neg_mask, int64_t* labels,
                                                                 float* label_weights, float* bbox_targets,
                                                                 float* bbox_weights) {
  const int b = blockIdx.y;
  const int Gb = gt_count(A.gt_counts, b, A.G);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < A.N; i += gridDim.x * 256) {
    const int64_t q = (int64_t)b * A.N + i;
    const bool p = pos_mask[q] != 0, n = neg_mask[q] != 0;
    f32x4_t t = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (p) {
      f32x4_t bx;
      fetch_box(A.S, b, i, Gb, &bx);
      const f32x4_t g = *(const f32x4_t*)(A.S.gt + ((int64_t)b * A.G + assigned[q] - 1) * 4);
      t = encode_box(bx, g, A.means, A.stds);
      w = (f32x4_t){1.f, 1.f, 1.f, 1.f};
    }
    labels[q] = p ? 1 : 0;
    label_weights[q] = (p || n) ? 1.f : 0.f;
    *(f32x4_t*)(bbox_targets + q * 4) = t;
    *(f32x4_t*)(bbox_weights + q * 4) = w;
  }
}

// one workgroup per image: ordered compaction of the sampled positives, then of the sampled negatives, then padding
__global__ __launch_bounds__(1024) void sample_rois_fill_kernel(const FillArgs A, const int32_t* __restrict__ assigned,
                                                                const uint8_t* __restrict__ pos_mask,
                                                                const uint8_t* __restrict__ neg_mask,
                                                                const int64_t* __restrict__ gt_labels,
                                                                float* rois, int64_t* labels, float* label_weights,
                                                                float* bbox_targets, float* bbox_weights,
                                                                int32_t* pos_gt_inds) {
  __shared__ int misc[TK_MISC];
  const int tid = threadIdx.x, b = blockIdx.x, N = A.N;
  const int Gb = gt_count(A.gt_counts, b, A.G);
  int done = 0;
  for (int cls = 0; cls < 2; ++cls) {
    const uint8_t* mrow = (cls ? neg_mask : pos_mask) + (int64_t)b * N;
    for (int base = 0; base < N; base += BLK) {
      const int i = base + tid;
      const bool f = i < N && mrow[i] != 0;
      int tot;
      const int row = done + block_excl_scan(f ? 1 : 0, misc, &tot);
      done += tot;
      if (f && row < A.num) {
        const int64_t r = (int64_t)b * A.num + row;
        f32x4_t bx, t = {0.f, 0.f, 0.f, 0.f};
        fetch_box(A.S, b, i, Gb, &bx);
        int64_t lab = 0;
        int gi = -1;
        if (cls == 0) {
          gi = assigned[(int64_t)b * N + i] - 1;
          t = encode_box(bx, *(const f32x4_t*)(A.S.gt + ((int64_t)b * A.G + gi) * 4), A.means, A.stds);
          lab = gt_labels[(int64_t)b * A.G + gi];
        }
        const float w = cls == 0 ? 1.f : 0.f;
        float* o = rois + r * 5;
        o[0] = (float)b;
        o[1] = bx[0];
        o[2] = bx[1];
        o[3] = bx[2];
        o[4] = bx[3];
        labels[r] = lab;
        label_weights[r] = 1.f;
        *(f32x4_t*)(bbox_targets + r * 4) = t;
        *(f32x4_t*)(bbox_weights + r * 4) = (f32x4_t){w, w, w, w};
        pos_gt_inds[r] = gi;
      }
    }
  }
  for (int row = done + tid; row < A.num; row += BLK) {
    const int64_t r = (int64_t)b * A.num + row;
    float* o = rois + r * 5;
    o[0] = -1.f;
    o[1] = o[2] = o[3] = o[4] = 0.f;
    labels[r] = 0;
    label_weights[r] = 0.f;
    *(f32x4_t*)(bbox_targets + r * 4) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    *(f32x4_t*)(bbox_weights + r * 4) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    pos_gt_inds[r] = -1;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------
// the ranges every entry point and every size query accepts
static int check_dims(const char* who, int B, int64_t N, int G) {
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(N >= 0 && N <= TDN_TARGET_MAX_BOXES, "%s: %lld boxes per image (max %d)", who, (long long)N,
            TDN_TARGET_MAX_BOXES);
  TDN_CHECK(G >= 0 && G <= TDN_TARGET_MAX_GT, "%s: G=%d ground truths per image (max %d)", who, G, TDN_TARGET_MAX_GT);
  return 0;
}
// sample_rois: P proposals leave room for the ground truths it may add
static int check_props(const char* who, int P) {
  TDN_CHECK(P >= 0 && P <= TDN_TARGET_MAX_BOXES - TDN_TARGET_MAX_GT, "%s: P=%d out of range", who, P);
  return 0;
}

static int check_common(const char* who, int B, int64_t N, int G, const tdn_target_config* cfg) {
  TDN_CHECK(cfg != nullptr, "%s: NULL config", who);
  if (check_dims(who, B, N, G) != 0) return -1;
  TDN_CHECK(cfg->pos_iou_thr == cfg->pos_iou_thr && cfg->neg_iou_thr == cfg->neg_iou_thr &&
                cfg->min_pos_iou == cfg->min_pos_iou, "%s: NaN threshold", who);
  return 0;
}

static int check_sampling(const char* who, const tdn_target_config* cfg) {
  TDN_CHECK(cfg->num >= 0 && cfg->num <= TDN_TARGET_MAX_NUM, "%s: num=%d out of 0..%d", who, cfg->num,
            TDN_TARGET_MAX_NUM);
  TDN_CHECK(cfg->num_pos_expected >= 0 && cfg->num_pos_expected <= cfg->num, "%s: num_pos_expected out of 0..num", who);
  TDN_CHECK(cfg->neg_pos_ub == cfg->neg_pos_ub, "%s: NaN neg_pos_ub", who);
  return 0;
}

// ---- workspaces (a braced list is evaluated left to right) ------------------------------------------------------
struct AssignWs { int64_t words; uint32_t* colmax; int* first; int64_t bytes; };   // `words` of each
static AssignWs assign_layout(int B, int G, void* base) {
  const int64_t words = (int64_t)B * (G > 0 ? G : 1);
  tdn_carver c{(char*)base, 0};
  return {words, c.take<uint32_t>(words), c.take<int>(words), c.off};
}
// anchor_target and sample_rois: the assignment words first, then assigned (sample_rois only: anchor_target's is an
// output of the call), then the two masks
struct SampleWs { AssignWs a; int32_t* assigned; uint8_t *pos_mask, *neg_mask; int64_t bytes; };
static SampleWs sample_layout(int B, int64_t N, int G, bool with_assigned, void* base) {
  const AssignWs a = assign_layout(B, G, base);
  const int64_t n = (int64_t)B * (N > 0 ? N : 1);
  tdn_carver c{(char*)base, a.bytes};
  return {a, with_assigned ? c.take<int32_t>(n) : nullptr, c.take<uint8_t>(n), c.take<uint8_t>(n), c.off};
}

static int run_assign(const BoxSrc& S, const int32_t* gt_counts, int B, int N, int G, const tdn_target_config* cfg,
                      int32_t* assigned, float* max_overlaps, const AssignWs& w, hipStream_t st) {
  AssignArgs A;
  A.S = S;
  A.gt_counts = gt_counts;
  A.N = N;
  A.G = G;
  A.all = cfg->gt_max_assign_all != 0;
  A.pos_thr = cfg->pos_iou_thr;
  A.neg_thr = cfg->neg_iou_thr;
  A.min_pos = cfg->min_pos_iou;
  TDN_LAUNCH(target_clear_kernel, dim3((int)((w.words + 255) / 256)), dim3(256), 0, st, w.colmax, w.first,
             (int)w.words);
  TDN_LAUNCH_CHECK();
  const dim3 grid((N + P1_THREADS * P1_PER - 1) / (P1_THREADS * P1_PER), B);
  TDN_LAUNCH(assign_pass1_kernel, grid, dim3(P1_THREADS), 0, st, A, assigned, max_overlaps, w.colmax);
  TDN_LAUNCH_CHECK();
  if (G == 0) return 0;                        // every participating box is already 0
  TDN_LAUNCH(assign_pass2_kernel, grid, dim3(P1_THREADS), 0, st, A, assigned, (const uint32_t*)w.colmax, w.first);
  TDN_LAUNCH_CHECK();
  if (!A.all) {
    TDN_LAUNCH(assign_first_kernel, dim3(B), dim3(MAXG), 0, st, (const int*)w.first, gt_counts, N, G, assigned);
    TDN_LAUNCH_CHECK();
  }
  return 0;
}

static BoxSrc anchor_src(const float* boxes, int64_t box_stride, const uint8_t* valid, int64_t valid_stride,
                         const float* gt, int G,
                         const int32_t* img_shapes, int border) {
  BoxSrc S;
  memset(&S, 0, sizeof(S));
  S.boxes = boxes;
  S.stride = box_stride;
  S.valid = valid;
  S.vstride = valid_stride;
  S.img_shapes = img_shapes;
  S.border = img_shapes ? border : -1;
  S.gt = gt;
  S.G = G;
  return S;
}

extern "C" int64_t tdn_assign_max_iou_workspace_bytes(int B, int G) {
  if (check_dims("tdn_assign_max_iou_workspace_bytes", B, 0, G) != 0) return -1;
  return assign_layout(B, G, nullptr).bytes;
}

extern "C" int tdn_assign_max_iou(const float* boxes, int64_t box_stride, const uint8_t* valid, int64_t valid_stride,
                                  const float* gt,
                                  const int32_t* gt_counts, int B, int N, int G, const tdn_target_config* cfg,
                                  int32_t* assigned, float* max_overlaps, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  if (check_common("tdn_assign_max_iou", B, N, G, cfg) != 0) return -1;
  TDN_CHECK(box_stride == 0 || box_stride >= (int64_t)N * 4, "tdn_assign_max_iou: bad box_stride");
  TDN_CHECK(valid_stride == 0 || valid_stride >= N, "tdn_assign_max_iou: bad valid_stride");
  if (N == 0) return 0;
  TDN_CHECK(boxes && gt_counts && assigned && workspace && (G == 0 || gt), "tdn_assign_max_iou: NULL pointer");
  const AssignWs w = assign_layout(B, G, workspace);
  if (tdn_check_ws("tdn_assign_max_iou", workspace, workspace_bytes, w.bytes) != 0) return -1;
  const BoxSrc S = anchor_src(boxes, box_stride, valid, valid_stride, gt, G, nullptr, -1);
  return run_assign(S, gt_counts, B, N, G, cfg, assigned, max_overlaps, w, (hipStream_t)stream);
}

static int run_select(const int32_t* assigned, int B, int N, const tdn_target_config* cfg, const int32_t* keys,
                      uint8_t* pos_mask, uint8_t* neg_mask, int32_t* num_pos, int32_t* num_neg, hipStream_t st) {
  SampleArgs A;
  A.N = N;
  A.num = cfg->num;
  A.num_pos_expected = cfg->num_pos_expected;
  A.neg_pos_ub = cfg->neg_pos_ub;
  A.seed = cfg->seed;
  TDN_LAUNCH(sample_select_kernel, dim3(2, B), dim3(BLK), 0, st, A, assigned, keys, pos_mask, neg_mask, num_pos,
             num_neg);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_sample_assigned(const int32_t* assigned, int B, int N, const tdn_target_config* cfg,
                                   const int32_t* keys, uint8_t* pos_mask, uint8_t* neg_mask, int32_t* num_pos,
                                   int32_t* num_neg, void* stream) {
  if (check_common("tdn_sample_assigned", B, N, 0, cfg) != 0 || check_sampling("tdn_sample_assigned", cfg) != 0)
    return -1;
  TDN_CHECK(num_pos && num_neg && (N == 0 || (assigned && pos_mask && neg_mask)), "tdn_sample_assigned: NULL pointer");
  return run_select(assigned, B, N, cfg, keys, pos_mask, neg_mask, num_pos, num_neg, (hipStream_t)stream);
}

extern "C" int64_t tdn_anchor_target_workspace_bytes(int B, int N, int G) {
  if (check_dims("tdn_anchor_target_workspace_bytes", B, N, G) != 0) return -1;
  return sample_layout(B, N, G, false, nullptr).bytes;
}

extern "C" int tdn_anchor_target(const float* anchors, int64_t box_stride, const uint8_t* valid, int64_t valid_stride,
                                 const float* gt,
                                 const int32_t* gt_counts, const int32_t* img_shapes, int B, int N, int G,
                                 const tdn_target_config* cfg, const int32_t* keys, int64_t* labels,
                                 float* label_weights, float* bbox_targets, float* bbox_weights, int32_t* num_pos,
                                 int32_t* num_neg, int32_t* assigned, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  if (check_common("tdn_anchor_target", B, N, G, cfg) != 0 || check_sampling("tdn_anchor_target", cfg) != 0) return -1;
  TDN_CHECK(box_stride == 0 || box_stride >= (int64_t)N * 4, "tdn_anchor_target: bad box_stride");
  TDN_CHECK(valid_stride == 0 || valid_stride >= N, "tdn_anchor_target: bad valid_stride");
  TDN_CHECK(gt_counts && num_pos && num_neg && workspace && (G == 0 || gt), "tdn_anchor_target: NULL pointer");
  TDN_CHECK(N == 0 || (anchors && labels && label_weights && bbox_targets && bbox_weights && assigned),
            "tdn_anchor_target: NULL pointer");
  TDN_CHECK(cfg->allowed_border < 0 || img_shapes, "tdn_anchor_target: allowed_border >= 0 needs img_shapes");
  const SampleWs w = sample_layout(B, N, G, false, workspace);
  if (tdn_check_ws("tdn_anchor_target", workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  const BoxSrc S = anchor_src(anchors, box_stride, valid, valid_stride, gt, G, img_shapes, cfg->allowed_border);
  if (N > 0 && run_assign(S, gt_counts, B, N, G, cfg, assigned, nullptr, w.a, st) != 0) return -1;
  if (run_select(assigned, B, N, cfg, keys, w.pos_mask, w.neg_mask, num_pos, num_neg, st) != 0) return -1;
  if (N == 0) return 0;
  FillArgs F;
  F.S = S;
  F.gt_counts = gt_counts;
  F.B = B;
  F.N = N;
  F.G = G;
  F.num = cfg->num;
  F.means = host_f4(cfg->means);
  F.stds = host_f4(cfg->stds);
  TDN_LAUNCH(anchor_target_fill_kernel, dim3(tdn_grid_1d(N, 256, 2048), B), dim3(256), 0, st, F,
             (const int32_t*)assigned, (const uint8_t*)w.pos_mask, (const uint8_t*)w.neg_mask, labels, label_weights,
             bbox_targets, bbox_weights);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_sample_rois_workspace_bytes(int B, int P, int G, int add_gt_as_proposals) {
  const char* who = "tdn_sample_rois_workspace_bytes";
  if (check_props(who, P) != 0 || check_dims(who, B, P, G) != 0) return -1;
  return sample_layout(B, (int64_t)P + (add_gt_as_proposals ? G : 0), G, true, nullptr).bytes;
}

extern "C" int tdn_sample_rois(const float* proposals, const int32_t* counts, const float* gt,
                               const int64_t* gt_labels, const int32_t* gt_counts, int B, int P, int G,
                               const tdn_target_config* cfg, const int32_t* keys, float* rois, int64_t* labels,
                               float* label_weights, float* bbox_targets, float* bbox_weights, int32_t* pos_gt_inds,
                               int32_t* num_pos, int32_t* num_neg, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  const char* who = "tdn_sample_rois";
  if (check_props(who, P) != 0 || check_common(who, B, P, G, cfg) != 0 || check_sampling(who, cfg) != 0) return -1;
  const int Nc = P + (cfg->add_gt_as_proposals ? G : 0);
  TDN_CHECK(gt_counts && counts && num_pos && num_neg && workspace && (G == 0 || (gt && gt_labels)) &&
                (P == 0 || proposals), "tdn_sample_rois: NULL pointer");
  TDN_CHECK(cfg->num == 0 || (rois && labels && label_weights && bbox_targets && bbox_weights && pos_gt_inds),
            "tdn_sample_rois: NULL output");
  const SampleWs w = sample_layout(B, Nc, G, true, workspace);
  if (tdn_check_ws("tdn_sample_rois", workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  BoxSrc S;
  memset(&S, 0, sizeof(S));
  S.cand = 1;
  S.props = proposals;
  S.counts = counts;
  S.P = P;
  S.add_gt = cfg->add_gt_as_proposals != 0;
  S.gt = gt;
  S.G = G;
  S.border = -1;
  if (Nc > 0 && run_assign(S, gt_counts, B, Nc, G, cfg, w.assigned, nullptr, w.a, st) != 0) return -1;
  if (run_select(w.assigned, B, Nc, cfg, keys, w.pos_mask, w.neg_mask, num_pos, num_neg, st) != 0) return -1;
  if (cfg->num == 0) return 0;
  FillArgs F;
  F.S = S;
  F.gt_counts = gt_counts;
  F.B = B;
  F.N = Nc;
  F.G = G;
  F.num = cfg->num;
  F.means = host_f4(cfg->means);
  F.stds = host_f4(cfg->stds);
  TDN_LAUNCH(sample_rois_fill_kernel, dim3(B), dim3(BLK), 0, st, F, (const int32_t*)w.assigned,
             (const uint8_t*)w.pos_mask, (const uint8_t*)w.neg_mask, gt_labels, rois, labels, label_weights, bbox_targets,
             bbox_weights, pos_gt_inds);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- IoU-balanced negative sampling -----------------------------------------------------------------
static int check_balanced(const char* who, const tdn_balanced_config* bal) {
  TDN_CHECK(bal != nullptr, "%s: NULL balanced config", who);
  TDN_CHECK(bal->num_bins >= 1 && bal->num_bins <= 8, "%s: num_bins=%d out of 1..8", who, bal->num_bins);
  TDN_CHECK(bal->floor_fraction >= 0.f && bal->floor_fraction <= 1.f, "%s: floor_fraction out of [0, 1]", who);
  TDN_CHECK(bal->floor_thr < 1.f, "%s: floor_thr must be below 1", who);
  return 0;
}

static int run_select_balanced(const int32_t* assigned, const float* overlaps, int B, int N, const tdn_target_config* cfg,
                               const tdn_balanced_config* bal, const int32_t* keys, uint8_t* pos_mask, uint8_t* neg_mask,
                               int32_t* num_pos, int32_t* num_neg, hipStream_t st) {
  SampleArgs A;
  A.N = N;
  A.num = cfg->num;
  A.num_pos_expected = cfg->num_pos_expected;
  A.neg_pos_ub = cfg->neg_pos_ub;
  A.seed = cfg->seed;
  const BalancedArgs Q{bal->floor_thr, bal->floor_fraction, bal->num_bins};
  TDN_LAUNCH(sample_select_balanced_kernel, dim3(2, B), dim3(BLK), 0, st, A, Q, assigned, overlaps, keys, pos_mask,
             neg_mask, num_pos, num_neg);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_sample_assigned_balanced(const int32_t* assigned, const float* max_overlaps, int B, int N,
                                            const tdn_target_config* cfg, const tdn_balanced_config* bal,
                                            const int32_t* keys, uint8_t* pos_mask, uint8_t* neg_mask, int32_t* num_pos,
                                            int32_t* num_neg, void* stream) {
  const char* who = "tdn_sample_assigned_balanced";
  if (check_common(who, B, N, 0, cfg) != 0 || check_sampling(who, cfg) != 0 || check_balanced(who, bal) != 0) return -1;
  TDN_CHECK(num_pos && num_neg && (N == 0 || (assigned && max_overlaps && pos_mask && neg_mask)), "%s: NULL pointer", who);
  return run_select_balanced(assigned, max_overlaps, B, N, cfg, bal, keys, pos_mask, neg_mask, num_pos, num_neg,
                             (hipStream_t)stream);
}

// tdn_sample_rois' workspace, then the candidates' max_overlaps
struct BalancedWs { SampleWs s; float* overlaps; int64_t bytes; };
static BalancedWs balanced_layout(int B, int64_t N, int G, void* base) {
  const SampleWs s = sample_layout(B, N, G, true, base);
  tdn_carver c{(char*)base, s.bytes};
  return {s, c.take<float>((int64_t)B * (N > 0 ? N : 1)), c.off};
}

extern "C" int64_t tdn_sample_rois_balanced_workspace_bytes(int B, int P, int G, int add_gt_as_proposals) {
  const char* who = "tdn_sample_rois_balanced_workspace_bytes";
  if (check_props(who, P) != 0 || check_dims(who, B, P, G) != 0) return -1;
  return balanced_layout(B, (int64_t)P + (add_gt_as_proposals ? G : 0), G, nullptr).bytes;
}

extern "C" int tdn_sample_rois_balanced(const float* proposals, const int32_t* counts, const float* gt,
                                        const int64_t* gt_labels, const int32_t* gt_counts, int B, int P, int G,
                                        const tdn_target_config* cfg, const tdn_balanced_config* bal, const int32_t* keys,
                                        float* rois, int64_t* labels, float* label_weights, float* bbox_targets,
                                        float* bbox_weights, int32_t* pos_gt_inds, int32_t* num_pos, int32_t* num_neg,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_sample_rois_balanced";
  if (check_props(who, P) != 0 || check_common(who, B, P, G, cfg) != 0 || check_sampling(who, cfg) != 0 ||
      check_balanced(who, bal) != 0)
    return -1;
  const int Nc = P + (cfg->add_gt_as_proposals ? G : 0);
  TDN_CHECK(gt_counts && counts && num_pos && num_neg && workspace && (G == 0 || (gt && gt_labels)) &&
                (P == 0 || proposals), "%s: NULL pointer", who);
  TDN_CHECK(cfg->num == 0 || (rois && labels && label_weights && bbox_targets && bbox_weights && pos_gt_inds),
            "%s: NULL output", who);
  const BalancedWs w = balanced_layout(B, Nc, G, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  BoxSrc S;
  memset(&S, 0, sizeof(S));
  S.cand = 1;
  S.props = proposals;
  S.counts = counts;
  S.P = P;
  S.add_gt = cfg->add_gt_as_proposals != 0;
  S.gt = gt;
  S.G = G;
  S.border = -1;
  if (Nc > 0 && run_assign(S, gt_counts, B, Nc, G, cfg, w.s.assigned, w.overlaps, w.s.a, st) != 0) return -1;
  if (run_select_balanced(w.s.assigned, w.overlaps, B, Nc, cfg, bal, keys, w.s.pos_mask, w.s.neg_mask, num_pos, num_neg,
                          st) != 0)
    return -1;
  if (cfg->num == 0) return 0;
  FillArgs F;
  F.S = S;
  F.gt_counts = gt_counts;
  F.B = B;
  F.N = Nc;
  F.G = G;
  F.num = cfg->num;
  F.means = host_f4(cfg->means);
  F.stds = host_f4(cfg->stds);
  TDN_LAUNCH(sample_rois_fill_kernel, dim3(B), dim3(BLK), 0, st, F, (const int32_t*)w.s.assigned,
             (const uint8_t*)w.s.pos_mask, (const uint8_t*)w.s.neg_mask, gt_labels, rois, labels, label_weights,
             bbox_targets, bbox_weights, pos_gt_inds);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- hooks for dense_detect.hip (target_host.h): the assignment of tdn_anchor_target on its own -------------------
#include "target_host.h"

// the assignment words padded to an even count, then `extra` more: the first launch clears all of them
static AssignWs assign_layout_extra(int B, int G, int64_t extra, void* base) {
  const int64_t words = (((int64_t)B * (G > 0 ? G : 1) + 1) & ~1ll) + extra;
  tdn_carver c{(char*)base, 0};
  return {words, c.take<uint32_t>(words), c.take<int>(words), c.off};
}

int64_t tdn_target_anchor_assign_bytes(int B, int G, int64_t extra_words) {
  return assign_layout_extra(B, G, extra_words, nullptr).bytes;
}

int tdn_target_anchor_assign(const char* who, const float* anchors, int64_t box_stride, const uint8_t* valid,
                             int64_t valid_stride, const float* gt, const int32_t* gt_counts, const int32_t* img_shapes,
                             int B, int N, int G, const tdn_target_config* cfg, int32_t* assigned, void* workspace,
                             int64_t extra_words, uint32_t** extra, void* stream) {
  if (check_common(who, B, N, G, cfg) != 0) return -1;
  TDN_CHECK(N >= 1, "%s: no anchors", who);
  TDN_CHECK(box_stride == 0 || box_stride >= (int64_t)N * 4, "%s: bad box_stride", who);
  TDN_CHECK(valid_stride == 0 || valid_stride >= N, "%s: bad valid_stride", who);
  TDN_CHECK(anchors && gt_counts && assigned && workspace && (G == 0 || gt), "%s: NULL pointer", who);
  TDN_CHECK(cfg->allowed_border < 0 || img_shapes, "%s: allowed_border >= 0 needs img_shapes", who);
  const AssignWs w = assign_layout_extra(B, G, extra_words, workspace);
  *extra = w.colmax + (w.words - extra_words);
  const BoxSrc S = anchor_src(anchors, box_stride, valid, valid_stride, gt, G, img_shapes, cfg->allowed_border);
  return run_assign(S, gt_counts, B, N, G, cfg, assigned, nullptr, w, (hipStream_t)stream);
}

// ---- hooks for guided.hip (target_host.h): launches 0 and 2b of the assignment on their own -------------------------
int tdn_target_clear(uint32_t* colmax, int* first, int64_t words, void* stream) {
  TDN_CHECK(words >= 1 && words <= 64ll * TDN_TARGET_MAX_GT, "tdn_target_clear: %lld words (1..B*G <= %d)",
            (long long)words, 64 * TDN_TARGET_MAX_GT);
  TDN_LAUNCH(target_clear_kernel, dim3((int)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, colmax, first,
             (int)words);
  TDN_LAUNCH_CHECK();
  return 0;
}

int tdn_target_assign_first(const int* first, const int32_t* gt_counts, int B, int N, int G, int32_t* assigned,
                            void* stream) {
  TDN_LAUNCH(assign_first_kernel, dim3(B), dim3(MAXG), 0, (hipStream_t)stream, first, gt_counts, N, G, assigned);
  TDN_LAUNCH_CHECK();
  return 0;
}
