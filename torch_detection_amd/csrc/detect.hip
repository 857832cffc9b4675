// Test-time detections of the RoI box head: softmax + decode, per-class NMS and the per-image top-k.
//
// Semantics are the project's own spec in the mmdetection-v0.x lineage (multiclass_nms / get_det_bboxes), '+1' boxes,
// strict IEEE fp32 in the spec's operation order (this file is compiled with -ffp-contract=off); the CPU restatement
// is tests/detect_ref.py.
//
// multiclass_nms is four launches for any B, C and N; bbox_head_detections puts one launch in front:
//   0 det_softmax_decode_kernel  one wavefront per RoI row: the softmax row of loss_roi_kernel (fp64 sum in the fixed
//                                lane -> column order) and the decode of every foreground class, written once as dense
//                                fp32 (R, C) scores and (R, 4C') boxes; everything after reads those.  The STAGES
//                                instantiation (cascade_detections, §4q) reads the logit as the mean of S matrices.
//   1 det_segment_kernel         one workgroup per (image, class): ordered compaction of the image's rows whose score
//                                in the class's column is > score_thr, LDS bitonic sort of (key << 32 | ~row), box
//                                gather into the segment's rows.  More than TDN_NMS_SEG_MAX candidates: count -1.
//   2 det_nms_mask_kernel        nms_mask_block of nms_core.h on every segment: grid (column block, row block, segment).
//   3 det_nms_scan_kernel        nms_scan_block of nms_core.h, one workgroup per segment; rows already are in key order.
//   4 det_merge_kernel           one workgroup per image: block_topk over the classes' survivors by (score key desc,
//                                class asc, row asc); writes the padded outputs and the count.
// With soft-NMS launches 2 and 3 are one:
//   2s det_soft_nms_kernel       soft_nms_segment of soft_nms_core.h, one workgroup per segment: the survivors in
//                                selection order, and every row's final score and its key, which the merge then reads.
// No memset, no float atomics, no inter-workgroup waits, no allocation; the integer LDS atomics of the radix select only
// count, so every output is a pure function of the inputs.
#include "nms_core.h"
#include "select_core.h"
#include "soft_nms_core.h"
#include "delta_core.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int DET_SEG_MAX = TDN_NMS_SEG_MAX;
constexpr int DET_WAVES = BLK / 64;
constexpr int DET_COLS = TDN_DET_MAX_CLASSES / 64;     // columns per lane of a row's wavefront

enum { IDX_NONE = 0, IDX_I32 = 1, IDX_I64 = 2, IDX_ROI = 3 };

// image of row r, or -1 for a row that takes no part.  IDX_ROI: column 0 of (R, 5) rois, by roi_align's rule (the
// truncated value must lie in [0, B); NaN does not)
__device__ __forceinline__ int row_image(const void* idx, int kind, int64_t r, int B) {
  if (kind == IDX_NONE) return 0;
  if (kind == IDX_ROI) {
    const float bf = ((const float*)idx)[r * 5];
    return (bf > -1.f && bf < (float)B) ? (int)bf : -1;
  }
  const long long v = kind == IDX_I32 ? (long long)((const int32_t*)idx)[r] : (long long)((const int64_t*)idx)[r];
  return (v >= 0 && v < B) ? (int)v : -1;
}

// ---- 0: softmax + decode, one wavefront per row -----------------------------------------------------------------
template <int DT> struct DetElem;
template <> struct DetElem<TDN_F32> { typedef float T; };
template <> struct DetElem<TDN_BF16> { typedef bf16_t T; };
template <> struct DetElem<TDN_F16> { typedef f16_t T; };

struct HeadArgs {
  const float* rois;          // (R, 5)
  const void* cls[TDN_CASCADE_MAX_STAGES];            // S matrices (R, C); bbox_head_detections: one
  int32_t S;
  const void* reg;            // (R, reg_cols)
  const int32_t* img_shapes;  // (B, 2)
  const float* scales;        // (B,) or null
  float scale;                // used when scales == null; 0: no rescale
  int32_t R, C, reg_cols, B;
  f32x4_t means, stds;
  float max_ratio;
};

// the logit of (r, c) at element offset i = r * C + c.  STAGES: (((x_0 + x_1) + ...) + x_{S-1}) / float(S), fp32
// additions in stage order and one fp32 division (S = 1 divides by 1: the value itself)
template <class T, bool STAGES>
__device__ __forceinline__ float head_logit(const HeadArgs& A, size_t i) {
  float v = (float)((const T*)A.cls[0])[i];
  if constexpr (STAGES) {
    for (int s = 1; s < A.S; ++s) v = __fadd_rn(v, (float)((const T*)A.cls[s])[i]);
    v = __fdiv_rn(v, (float)A.S);
  }
  return v;
}

template <int DT, bool STAGES>
__global__ __launch_bounds__(BLK) void det_softmax_decode_kernel(const HeadArgs A, float* __restrict__ scores,
                                                                 float* __restrict__ boxes) {
  typedef typename DetElem<DT>::T T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = A.C;
  const int nbox = A.reg_cols == 4 ? 1 : C - 1;       // boxes per row of the dense output
  for (int r = blockIdx.x * DET_WAVES + wave; r < A.R; r += gridDim.x * DET_WAVES) {
    const float* roi = A.rois + (size_t)r * 5;
    const int b = row_image(A.rois, IDX_ROI, r, A.B);           // wave-uniform
    float* sr = scores + (size_t)r * C;
    f32x4_t* br = (f32x4_t*)boxes + (size_t)r * nbox;
    if (b < 0) {
      for (int c = lane; c < C; c += 64) sr[c] = 0.f;
      for (int c = lane; c < nbox; c += 64) br[c] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      continue;
    }
    // softmax: the row of loss_roi_kernel, operation for operation
    float x[DET_COLS];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < DET_COLS; ++j) {
      const int c = lane + 64 * j;
      x[j] = c < C ? head_logit<T, STAGES>(A, (size_t)r * C + c) : -INFINITY;
      m = fmaxf(m, x[j]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    double sd = 0.0;
#pragma unroll
    for (int j = 0; j < DET_COLS; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        x[j] = expf(__fsub_rn(x[j], m));
        sd += (double)x[j];
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sd += __shfl_xor(sd, o);
    const float S = (float)sd;
#pragma unroll
    for (int j = 0; j < DET_COLS; ++j) {
      const int c = lane + 64 * j;
      if (c < C) sr[c] = __fdiv_rn(x[j], S);
    }
    // decode: box k of the row from delta columns 4(k+1).. (class-specific) or 0.. (class-agnostic)
    const f32x4_t rb = {roi[1], roi[2], roi[3], roi[4]};
    const int ih = A.img_shapes[2 * b], iw = A.img_shapes[2 * b + 1];
    const float sc = A.scales ? A.scales[b] : A.scale;
    const T* dr = (const T*)A.reg + (size_t)r * A.reg_cols + (A.reg_cols == 4 ? 0 : 4);
    for (int k = lane; k < nbox; k += 64) {
      f32x4_t d;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = (float)dr[4 * k + e];
      f32x4_t o = decode_box(rb, d, A.means, A.stds, A.max_ratio, ih, iw);
      if (A.scales || A.scale != 0.f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fdiv_rn(o[e], sc);
      }
      br[k] = o;
    }
  }
}

// ---- 1: the (image, class) segments -----------------------------------------------------------------------------
struct DetArgs {
  const float* boxes;         // (N, box_cols)
  const float* scores;        // (N, C)
  const void* idx;            // image of each row
  int32_t idx_kind;
  int32_t N, C, B, box_cols;
  int32_t cap, pitch, max_num;
  float score_thr, nms_thr;
};

constexpr size_t SEG_LDS = (size_t)DET_SEG_MAX * 8 + TK_MISC * 4;                               // 33 KB

__global__ __launch_bounds__(BLK) void det_segment_kernel(const DetArgs A, f32x4_t* seg_box, uint32_t* seg_key,
                                                          int* seg_row, int* seg_start, int* seg_count) {
  extern __shared__ __attribute__((aligned(16))) u64 smem[];
  u64* skeys = smem;                                  // [DET_SEG_MAX]
  int* misc = (int*)(smem + DET_SEG_MAX);             // [TK_MISC]
  const int tid = threadIdx.x;
  const int s = blockIdx.x, Cf = A.C - 1;
  const int b = s / Cf, cls = s - b * Cf + 1;         // score column of the class
  const int start = s * A.cap;
  // candidates in row order; a thread takes TK_PER consecutive rows, so one scan orders a whole step
  int n = 0;
  for (int base = 0; base < A.N; base += TK_STEP) {
    const int r0 = base + tid * TK_PER;
    uint32_t key[TK_PER];
    unsigned cand = 0u;                               // bit e: row r0 + e is a candidate
#pragma unroll
    for (int e = 0; e < TK_PER; ++e) {
      const int r = r0 + e;
      key[e] = 0u;
      if (r < A.N && row_image(A.idx, A.idx_kind, r, A.B) == b) {
        const float sc = A.scores[(size_t)r * A.C + cls];
        key[e] = order_key(sc);
        cand |= sc > A.score_thr ? 1u << e : 0u;
      }
    }
    int tot;
    int pos = n + block_excl_scan(__builtin_popcount(cand), misc, &tot);
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (cand >> e & 1u) {
        if (pos < DET_SEG_MAX) skeys[pos] = compose(key[e], (uint32_t)(r0 + e));
        ++pos;
      }
    n += tot;
  }
  if (n > DET_SEG_MAX || n > A.cap) {                 // the second cannot happen: cap = min(N, DET_SEG_MAX)
    if (tid == 0) {
      seg_start[s] = start;
      seg_count[s] = -1;
    }
    return;
  }
  const int P = pow2_ceil(n);
  for (int i = n + tid; i < P; i += BLK) skeys[i] = 0ull;       // below every real key
  block_sort_desc(skeys, P);
  const int col = A.box_cols == 4 ? 0 : 4 * (cls - 1);
  for (int p = tid; p < n; p += BLK) {
    const u64 c = skeys[p];
    const int r = (int)~(uint32_t)c;
    seg_box[start + p] = *(const f32x4_t*)(A.boxes + (size_t)r * A.box_cols + col);
    seg_key[start + p] = (uint32_t)(c >> 32);
    seg_row[start + p] = r;
  }
  if (tid == 0) {
    seg_start[s] = start;
    seg_count[s] = n;
  }
}

// ---- 2, 3: NMS of every segment (the bodies are nms_core.h's) --------------------------------------------------------
__global__ __launch_bounds__(64) void det_nms_mask_kernel(const float* __restrict__ sboxes, const int* seg_start,
                                                          const int* seg_count, float thr, int pitch,
                                                          unsigned long long* __restrict__ mask) {
  const int s = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;
  const int n = seg_count[s];
  if (cb * 64 >= n) return;                           // also n <= 0; rb <= cb
  const int64_t start = seg_start[s];
  nms_mask_block(sboxes + start * 4, n, thr, pitch, rb, cb, mask + start * pitch);
}

// kept[start + j]: the segment-local row of survivor j; num_kept[s] = survivors, -1 for an oversized segment
__global__ __launch_bounds__(BLK) void det_nms_scan_kernel(const unsigned long long* __restrict__ mask,
                                                           const int* seg_start, const int* seg_count, int pitch,
                                                           int64_t* kept, int* num_kept) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sm[];
  const int s = blockIdx.x;
  const int n = seg_count[s];
  if (n <= 0) {
    if (threadIdx.x == 0) num_kept[s] = n < 0 ? -1 : 0;
    return;
  }
  const int64_t start = seg_start[s];
  nms_scan_block(mask + start * pitch, nullptr, n, (n + 63) / 64, pitch, nullptr, kept + start, num_kept + s, sm);
}

// ---- 2s: soft-NMS of every segment (the body is soft_nms_core.h's) -----------------------------------------------------
// seg_key is rewritten in place: on return seg_key[r] / seg_score[r] are the final score's key / the final score of row r
__global__ __launch_bounds__(BLK) void det_soft_nms_kernel(const DetArgs A, const SoftArgs P,
                                                           const f32x4_t* __restrict__ seg_box,
                                                           const int* __restrict__ seg_row, const int* seg_start,
                                                           const int* seg_count, uint32_t* seg_key, float* seg_score,
                                                           int64_t* kept, int* num_kept) {
  __shared__ SoftLds sh;
  const int s = blockIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(seg_count[s]);
  if (n <= 0) {
    if (threadIdx.x == 0) num_kept[s] = n < 0 ? -1 : 0;
    return;
  }
  const int64_t start = seg_start[s];
  const int Cf = A.C - 1;
  const float* scol = A.scores + (s - (s / Cf) * Cf + 1);       // the class's column
  if (n <= SOFT_WAVE_MAX) {
    if (threadIdx.x >= 64) return;                    // no barrier is reached on this path
    soft_nms_segment<true>(P, seg_box + start, seg_row + start, scol, A.C, n, seg_key + start, seg_score + start,
                           kept + start, num_kept + s, &sh);
  } else {
    soft_nms_segment<false>(P, seg_box + start, seg_row + start, scol, A.C, n, seg_key + start, seg_score + start,
                            kept + start, num_kept + s, &sh);
  }
}

// ---- 4: per image, the best max_num of the classes' survivors ------------------------------------------------------
// candidate j of an image: survivor j - cum[c] of class c, classes in order; among equal keys the candidate order is
// (class asc, row asc), because a segment's survivors keep its (key desc, row asc) order
struct SurvivorFetch {
  const int* cum;           // [Cf + 1] LDS
  int Cf, seg0, cap;
  const int64_t* kept;
  const uint32_t* seg_key;
  __device__ __forceinline__ int cls(int j) const {   // the last c with cum[c] <= j
    int lo = 0, hi = Cf - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cum[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
  }
  __device__ __forceinline__ int row(int j, int c) const {      // row of the segment arrays
    const int st = (seg0 + c) * cap;
    return st + (int)kept[st + j - cum[c]];
  }
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (e < cnt) kk[e] = seg_key[row(i0 + e, cls(i0 + e))];
  }
};

// dynamic LDS of det_merge_kernel: sorted keys, radix histogram, scratch, class offsets
size_t merge_lds(int max_num, int C) {
  return (size_t)pow2_ceil(max_num) * 8 + TK_BINS * 4 + TK_MISC * 4 + (size_t)(C + 1) * 4;
}

// SOFT: seg_key holds the final scores' keys and A.scores IS the per-row array of final scores (det_run_soft)
template <bool SOFT>
__global__ __launch_bounds__(BLK) void det_merge_kernel(const DetArgs A, const f32x4_t* __restrict__ seg_box,
                                                        const uint32_t* __restrict__ seg_key,
                                                        const int* __restrict__ seg_row,
                                                        const int64_t* __restrict__ kept, const int* num_kept,
                                                        float* dets, int64_t* labels, int64_t* row_idx,
                                                        int32_t* counts) {
  extern __shared__ __attribute__((aligned(16))) u64 smem[];
  const int K = pow2_ceil(A.max_num);
  u64* skeys = smem;                                  // [K]
  int* hist = (int*)(smem + K);                       // [TK_BINS]
  int* misc = hist + TK_BINS;                         // [TK_MISC]
  int* cum = misc + TK_MISC;                          // [Cf + 1]
  const int tid = threadIdx.x, b = blockIdx.x, Cf = A.C - 1;
  // class offsets: Cf <= 1023 survivors' counts, one per thread; an oversized segment empties the image
  const int nk = tid < Cf ? num_kept[b * Cf + tid] : 0;
  const int bad = __syncthreads_or(nk < 0);
  int T;
  const int ex = block_excl_scan(nk < 0 ? 0 : nk, misc, &T);
  if (tid < Cf) cum[tid] = ex;
  if (tid == 0) cum[Cf] = T;
  __syncthreads();
  int m = 0;
  const SurvivorFetch F{cum, Cf, b * Cf, A.cap, kept, seg_key};
  if (!bad) m = block_topk(F, T, min(A.max_num, T), skeys, hist, misc);
  for (int p = tid; p < A.max_num; p += BLK) {
    float* o = dets + ((int64_t)b * A.max_num + p) * 5;
    const int64_t q = (int64_t)b * A.max_num + p;
    if (p < m) {
      const int j = (int)~(uint32_t)skeys[p];
      const int c = F.cls(j);
      const int r = F.row(j, c);
      const f32x4_t bx = seg_box[r];
      const int src = seg_row[r];
      o[0] = bx[0];
      o[1] = bx[1];
      o[2] = bx[2];
      o[3] = bx[3];
      if constexpr (SOFT) o[4] = A.scores[r];
      else o[4] = A.scores[(size_t)src * A.C + c + 1];     // the stored score itself (-0.0 stays -0.0)
      labels[q] = c;
      row_idx[q] = src;
    } else {
#pragma unroll
      for (int e = 0; e < 5; ++e) o[e] = 0.f;
      labels[q] = -1;
      row_idx[q] = -1;
    }
  }
  if (tid == 0) counts[b] = bad ? -1 : m;
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct DetPlan {
  DetArgs A;
  int S;
  int64_t rows;
};

// the checks both the query and the call depend on
int det_plan(const char* who, int N, int C, int B, DetPlan* out) {
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(C >= 2 && C <= TDN_DET_MAX_CLASSES, "%s: C=%d out of 2..%d", who, C, TDN_DET_MAX_CLASSES);
  TDN_CHECK(N >= 0 && N <= TDN_DET_MAX_ROWS, "%s: %d rows (max %d)", who, N, TDN_DET_MAX_ROWS);
  memset(&out->A, 0, sizeof(out->A));
  DetArgs& A = out->A;
  A.N = N;
  A.C = C;
  A.B = B;
  A.cap = N < DET_SEG_MAX ? (N > 0 ? N : 1) : DET_SEG_MAX;    // no rows: one placeholder row per segment
  A.pitch = (A.cap + 63) / 64;
  out->S = B * (C - 1);
  out->rows = (int64_t)out->S * A.cap;
  return 0;
}

struct DetWs {
  f32x4_t* seg_box; uint32_t* seg_key; int* seg_row; int64_t* kept;
  int *seg_start, *seg_count, *num_kept; u64* mask; int64_t bytes;
};
DetWs det_layout(const DetPlan& p, void* base) {   // a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<f32x4_t>(p.rows), c.take<uint32_t>(p.rows), c.take<int>(p.rows), c.take<int64_t>(p.rows),
          c.take<int>(p.S), c.take<int>(p.S), c.take<int>(p.S), c.take<u64>(p.rows * p.A.pitch), c.off};
}

// soft-NMS: no mask, the rows' final scores instead
struct SoftWs {
  f32x4_t* seg_box; uint32_t* seg_key; int* seg_row; int64_t* kept; float* seg_score;
  int *seg_start, *seg_count, *num_kept; int64_t bytes;
};
SoftWs soft_layout(const DetPlan& p, void* base) {   // a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<f32x4_t>(p.rows), c.take<uint32_t>(p.rows), c.take<int>(p.rows), c.take<int64_t>(p.rows),
          c.take<float>(p.rows), c.take<int>(p.S), c.take<int>(p.S), c.take<int>(p.S), c.off};
}

int det_run_soft(const char* who, DetPlan& p, float score_thr, const tdn_soft_nms_config* soft, int max_num,
                 float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                 int64_t workspace_bytes, void* stream);

// launches 1..4 on dense fp32 boxes and scores; soft != null: launches 1, 2s, 4
int det_run(const char* who, DetPlan& p, float score_thr, float nms_thr, int max_num, float* dets, int64_t* labels,
            int64_t* row_idx, int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream,
            const tdn_soft_nms_config* soft = nullptr) {
  if (soft) return det_run_soft(who, p, score_thr, soft, max_num, dets, labels, row_idx, counts, workspace,
                                workspace_bytes, stream);
  TDN_CHECK(max_num >= 1 && max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, max_num, TDN_RPN_MAX_NUM);
  TDN_CHECK(score_thr - score_thr == 0.f && nms_thr - nms_thr == 0.f, "%s: score_thr / nms_thr must be finite", who);
  TDN_CHECK(dets && labels && row_idx && counts, "%s: NULL output", who);
  TDN_CHECK(p.rows < (1ll << 31), "%s: B * (C - 1) * min(N, %d) segment rows do not fit 31 bits", who, DET_SEG_MAX);
  DetArgs& A = p.A;
  A.score_thr = score_thr;
  A.nms_thr = nms_thr;
  A.max_num = max_num;
  const DetWs w = det_layout(p, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  TDN_LAUNCH(det_segment_kernel, dim3(p.S), dim3(BLK), SEG_LDS, st, A, w.seg_box, w.seg_key, w.seg_row, w.seg_start,
             w.seg_count);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(det_nms_mask_kernel, dim3(A.pitch, A.pitch, p.S), dim3(64), 0, st, (const float*)w.seg_box,
             (const int*)w.seg_start, (const int*)w.seg_count, nms_thr, A.pitch, w.mask);
  TDN_LAUNCH_CHECK();
  if (tdn_allow_lds<det_nms_scan_kernel>(160 * 1024, "det_nms_scan") < 0) return -1;
  TDN_LAUNCH(det_nms_scan_kernel, dim3(p.S), dim3(BLK), nms_scan_block_lds(A.pitch), st,
             (const unsigned long long*)w.mask, (const int*)w.seg_start, (const int*)w.seg_count, A.pitch, w.kept,
             w.num_kept);
  TDN_LAUNCH_CHECK();
  // at most 78 KB (max_num = 8192, C = 1024); the kernel also has a few static bytes, so not the full 160 KB
  if (tdn_allow_lds<det_merge_kernel<false>>((int)merge_lds(TDN_RPN_MAX_NUM, TDN_DET_MAX_CLASSES), "det_merge") < 0)
    return -1;
  TDN_LAUNCH(det_merge_kernel<false>, dim3(A.B), dim3(BLK), merge_lds(max_num, A.C), st, A, (const f32x4_t*)w.seg_box,
             (const uint32_t*)w.seg_key, (const int*)w.seg_row, (const int64_t*)w.kept, (const int*)w.num_kept, dets,
             labels, row_idx, counts);
  TDN_LAUNCH_CHECK();
  return 0;
}

int det_run_soft(const char* who, DetPlan& p, float score_thr, const tdn_soft_nms_config* soft, int max_num,
                 float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                 int64_t workspace_bytes, void* stream) {
  if (tdn_soft_nms_check(who, soft) != 0) return -1;
  TDN_CHECK(max_num >= 1 && max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, max_num, TDN_RPN_MAX_NUM);
  TDN_CHECK(score_thr - score_thr == 0.f, "%s: score_thr must be finite", who);
  TDN_CHECK(dets && labels && row_idx && counts, "%s: NULL output", who);
  TDN_CHECK(p.rows < (1ll << 31), "%s: B * (C - 1) * min(N, %d) segment rows do not fit 31 bits", who, DET_SEG_MAX);
  DetArgs& A = p.A;
  A.score_thr = score_thr;
  A.nms_thr = soft->iou_thr;
  A.max_num = max_num;
  const SoftArgs P{soft->method, soft->iou_thr, soft->sigma, soft->min_score};
  const SoftWs w = soft_layout(p, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  TDN_LAUNCH(det_segment_kernel, dim3(p.S), dim3(BLK), SEG_LDS, st, A, w.seg_box, w.seg_key, w.seg_row, w.seg_start,
             w.seg_count);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(det_soft_nms_kernel, dim3(p.S), dim3(BLK), 0, st, A, P, (const f32x4_t*)w.seg_box, (const int*)w.seg_row,
             (const int*)w.seg_start, (const int*)w.seg_count, w.seg_key, w.seg_score, w.kept, w.num_kept);
  TDN_LAUNCH_CHECK();
  DetArgs M = A;                                      // the merge reads a row's score at scores[row of the segment arrays]
  M.scores = w.seg_score;
  if (tdn_allow_lds<det_merge_kernel<true>>((int)merge_lds(TDN_RPN_MAX_NUM, TDN_DET_MAX_CLASSES), "det_merge_soft") < 0)
    return -1;
  TDN_LAUNCH(det_merge_kernel<true>, dim3(A.B), dim3(BLK), merge_lds(max_num, A.C), st, M, (const f32x4_t*)w.seg_box,
             (const uint32_t*)w.seg_key, (const int*)w.seg_row, (const int64_t*)w.kept, (const int*)w.num_kept, dets,
             labels, row_idx, counts);
  TDN_LAUNCH_CHECK();
  return 0;
}

int64_t det_ws_query(const char* who, int N, int C, int B, bool soft) {
  DetPlan p;
  if (det_plan(who, N, C, B, &p) != 0) return -1;
  return soft ? soft_layout(p, nullptr).bytes : det_layout(p, nullptr).bytes;
}

}  // namespace

extern "C" int64_t tdn_multiclass_nms_workspace_bytes(int N, int C, int B) {
  return det_ws_query("tdn_multiclass_nms", N, C, B, false);
}
extern "C" int64_t tdn_multiclass_nms_soft_workspace_bytes(int N, int C, int B) {
  return det_ws_query("tdn_multiclass_nms_soft", N, C, B, true);
}

namespace {
int multiclass_run(const char* who, const float* boxes, int box_cols, const float* scores, const void* batch_idx,
                   int batch_idx_bytes, int N, int C, int B, float score_thr, float nms_thr,
                   const tdn_soft_nms_config* soft, int max_num, float* dets, int64_t* labels, int64_t* row_idx,
                   int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  DetPlan p;
  if (det_plan(who, N, C, B, &p) != 0) return -1;
  TDN_CHECK(box_cols == 4 || box_cols == 4 * (C - 1), "%s: box_cols=%d is neither 4 nor 4 * (C - 1)", who, box_cols);
  TDN_CHECK(batch_idx ? (batch_idx_bytes == 4 || batch_idx_bytes == 8) : (B == 1 || N == 0),
            "%s: batch_idx must be int32 or int64, or NULL for one image", who);
  TDN_CHECK(N == 0 || (boxes && scores), "%s: NULL boxes / scores", who);
  p.A.boxes = boxes;
  p.A.scores = scores;
  p.A.idx = batch_idx;
  p.A.idx_kind = !batch_idx ? IDX_NONE : (batch_idx_bytes == 4 ? IDX_I32 : IDX_I64);
  p.A.box_cols = box_cols;
  return det_run(who, p, score_thr, nms_thr, max_num, dets, labels, row_idx, counts, workspace, workspace_bytes, stream,
                 soft);
}
}  // namespace

extern "C" int tdn_multiclass_nms(const float* boxes, int box_cols, const float* scores, const void* batch_idx,
                                  int batch_idx_bytes, int N, int C, int B, float score_thr, float nms_thr,
                                  int max_num, float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return multiclass_run("tdn_multiclass_nms", boxes, box_cols, scores, batch_idx, batch_idx_bytes, N, C, B, score_thr,
                        nms_thr, nullptr, max_num, dets, labels, row_idx, counts, workspace, workspace_bytes, stream);
}

extern "C" int tdn_multiclass_nms_soft(const float* boxes, int box_cols, const float* scores, const void* batch_idx,
                                       int batch_idx_bytes, int N, int C, int B, float score_thr,
                                       const tdn_soft_nms_config* soft, int max_num, float* dets, int64_t* labels,
                                       int64_t* row_idx, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
  const char* who = "tdn_multiclass_nms_soft";
  if (tdn_soft_nms_check(who, soft) != 0) return -1;
  return multiclass_run(who, boxes, box_cols, scores, batch_idx, batch_idx_bytes, N, C, B, score_thr, 0.f, soft,
                        max_num, dets, labels, row_idx, counts, workspace, workspace_bytes, stream);
}

extern "C" int64_t tdn_bbox_detections_workspace_bytes(int R, int C, int B) {
  return det_ws_query("tdn_bbox_detections", R, C, B, false);
}
extern "C" int64_t tdn_bbox_detections_soft_workspace_bytes(int R, int C, int B) {
  return det_ws_query("tdn_bbox_detections_soft", R, C, B, true);
}
extern "C" int64_t tdn_cascade_detections_soft_workspace_bytes(int R, int C, int B) {
  return det_ws_query("tdn_cascade_detections_soft", R, C, B, true);
}

namespace {

template <bool STAGES>
void head_launch(int dtype, dim3 grid, void* stream, const HeadArgs& H, float* dense_scores, float* dense_boxes) {
  const dim3 block(BLK);
  if (dtype == TDN_F32) TDN_LAUNCH((det_softmax_decode_kernel<TDN_F32, STAGES>), grid, block, 0, stream, H, dense_scores, dense_boxes);
  else if (dtype == TDN_BF16) TDN_LAUNCH((det_softmax_decode_kernel<TDN_BF16, STAGES>), grid, block, 0, stream, H, dense_scores, dense_boxes);
  else TDN_LAUNCH((det_softmax_decode_kernel<TDN_F16, STAGES>), grid, block, 0, stream, H, dense_scores, dense_boxes);
}

// tdn_bbox_detections (stages = false: cls[0] read as it is) and tdn_cascade_detections (stages = true: the mean of S)
int head_detections(const char* who, bool stages, const float* rois, const void* const* cls, int S, const void* reg,
                    int dtype, int R, int C, int reg_cols, int B, const int32_t* img_shapes, const float* scale_factors,
                    float scale_factor, const float* means4, const float* stds4, double wh_ratio_clip, float score_thr,
                    float nms_thr, int max_num, float* dense_scores, float* dense_boxes, float* dets, int64_t* labels,
                    int64_t* row_idx, int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream,
                    const tdn_soft_nms_config* soft = nullptr) {
  if (soft && tdn_soft_nms_check(who, soft) != 0) return -1;  // before the first launch
  DetPlan p;
  if (det_plan(who, R, C, B, &p) != 0) return -1;
  TDN_CHECK(dtype == TDN_F32 || dtype == TDN_BF16 || dtype == TDN_F16, "%s: dtype %d", who, dtype);
  TDN_CHECK(reg_cols == 4 || reg_cols == 4 * C, "%s: reg_cols=%d is neither 4 nor 4 * C", who, reg_cols);
  TDN_CHECK(means4 && stds4 && img_shapes, "%s: NULL means / stds / img_shapes", who);
  TDN_CHECK(wh_ratio_clip > 0.0 && wh_ratio_clip < 1.0, "%s: wh_ratio_clip must be in (0, 1)", who);
  TDN_CHECK(scale_factors || scale_factor == 0.f || (scale_factor > 0.f && scale_factor - scale_factor == 0.f),
            "%s: scale_factor must be positive and finite (0: none)", who);
  TDN_CHECK(R == 0 || (rois && reg && dense_scores && dense_boxes), "%s: NULL pointer", who);
  HeadArgs H;
  memset(&H, 0, sizeof(H));
  H.rois = rois;
  for (int s = 0; s < S; ++s) {
    TDN_CHECK(R == 0 || cls[s], "%s: NULL pointer", who);
    H.cls[s] = cls[s];
  }
  H.S = S;
  H.reg = reg;
  H.img_shapes = img_shapes;
  H.scales = scale_factors;
  H.scale = scale_factors ? 0.f : scale_factor;
  H.R = R;
  H.C = C;
  H.reg_cols = reg_cols;
  H.B = B;
  H.means = host_f4(means4);
  H.stds = host_f4(stds4);
  H.max_ratio = (float)fabs(log(wh_ratio_clip));     // as tdn_delta2bbox: in double, rounded to fp32
  if (R > 0) {
    const dim3 grid(tdn_grid_1d(R, DET_WAVES, 4096));
    if (stages) head_launch<true>(dtype, grid, stream, H, dense_scores, dense_boxes);
    else head_launch<false>(dtype, grid, stream, H, dense_scores, dense_boxes);
    TDN_LAUNCH_CHECK();
  }
  p.A.boxes = dense_boxes;
  p.A.scores = dense_scores;
  p.A.idx = rois;
  p.A.idx_kind = IDX_ROI;
  p.A.box_cols = reg_cols == 4 ? 4 : 4 * (C - 1);
  return det_run(who, p, score_thr, nms_thr, max_num, dets, labels, row_idx, counts, workspace, workspace_bytes, stream,
                 soft);
}

}  // namespace

extern "C" int tdn_bbox_detections(const float* rois, const void* cls, const void* reg, int dtype, int R, int C,
                                   int reg_cols, int B, const int32_t* img_shapes, const float* scale_factors,
                                   float scale_factor, const float* means4, const float* stds4, double wh_ratio_clip,
                                   float score_thr, float nms_thr, int max_num, float* dense_scores, float* dense_boxes,
                                   float* dets, int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  return head_detections("tdn_bbox_detections", false, rois, &cls, 1, reg, dtype, R, C, reg_cols, B, img_shapes,
                         scale_factors, scale_factor, means4, stds4, wh_ratio_clip, score_thr, nms_thr, max_num,
                         dense_scores, dense_boxes, dets, labels, row_idx, counts, workspace, workspace_bytes, stream);
}

extern "C" int tdn_cascade_detections(const float* rois, const void* const* cls, int num_stages, const void* reg,
                                      int dtype, int R, int C, int reg_cols, int B, const int32_t* img_shapes,
                                      const float* scale_factors, float scale_factor, const float* means4,
                                      const float* stds4, double wh_ratio_clip, float score_thr, float nms_thr,
                                      int max_num, float* dense_scores, float* dense_boxes, float* dets,
                                      int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_cascade_detections";
  TDN_CHECK(cls && num_stages >= 1 && num_stages <= TDN_CASCADE_MAX_STAGES, "%s: %d stages (1..%d)", who, num_stages,
            TDN_CASCADE_MAX_STAGES);
  return head_detections(who, true, rois, cls, num_stages, reg, dtype, R, C, reg_cols, B, img_shapes, scale_factors,
                         scale_factor, means4, stds4, wh_ratio_clip, score_thr, nms_thr, max_num, dense_scores,
                         dense_boxes, dets, labels, row_idx, counts, workspace, workspace_bytes, stream);
}

extern "C" int tdn_bbox_detections_soft(const float* rois, const void* cls, const void* reg, int dtype, int R, int C,
                                        int reg_cols, int B, const int32_t* img_shapes, const float* scale_factors,
                                        float scale_factor, const float* means4, const float* stds4,
                                        double wh_ratio_clip, float score_thr, const tdn_soft_nms_config* soft,
                                        int max_num, float* dense_scores, float* dense_boxes, float* dets,
                                        int64_t* labels, int64_t* row_idx, int32_t* counts, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_bbox_detections_soft";
  if (tdn_soft_nms_check(who, soft) != 0) return -1;
  return head_detections(who, false, rois, &cls, 1, reg, dtype, R, C, reg_cols, B, img_shapes, scale_factors,
                         scale_factor, means4, stds4, wh_ratio_clip, score_thr, 0.f, max_num, dense_scores, dense_boxes,
                         dets, labels, row_idx, counts, workspace, workspace_bytes, stream, soft);
}

extern "C" int tdn_cascade_detections_soft(const float* rois, const void* const* cls, int num_stages, const void* reg,
                                           int dtype, int R, int C, int reg_cols, int B, const int32_t* img_shapes,
                                           const float* scale_factors, float scale_factor, const float* means4,
                                           const float* stds4, double wh_ratio_clip, float score_thr,
                                           const tdn_soft_nms_config* soft, int max_num, float* dense_scores,
                                           float* dense_boxes, float* dets, int64_t* labels, int64_t* row_idx,
                                           int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_cascade_detections_soft";
  if (tdn_soft_nms_check(who, soft) != 0) return -1;
  TDN_CHECK(cls && num_stages >= 1 && num_stages <= TDN_CASCADE_MAX_STAGES, "%s: %d stages (1..%d)", who, num_stages,
            TDN_CASCADE_MAX_STAGES);
  return head_detections(who, true, rois, cls, num_stages, reg, dtype, R, C, reg_cols, B, img_shapes, scale_factors,
                         scale_factor, means4, stds4, wh_ratio_clip, score_thr, 0.f, max_num, dense_scores, dense_boxes,
                         dets, labels, row_idx, counts, workspace, workspace_bytes, stream, soft);
}

// ---- box refinement between the stages of a cascade ---------------------------------------------------
// Row r of (R, 5) rois decodes against the deltas of ONE class: its label (given, or the arg-max of its class logits).
//   row-aligned  one launch, one thread per row, 256 rows per workgroup: row r of the output is [image, box] or
//                [-1, 0, 0, 0, 0].
//   compacted    two launches over chunks of REFINE_CHUNK = 1024 rows, one workgroup each, one thread per row:
//     0 refine_count_kernel  kept rows of every image in the chunk -> chunk_cnt[chunk][B] (the workspace)
//     1 refine_kernel        every workgroup sums chunk_cnt over the chunks before it (its images' first output rows)
//                            and over all chunks (the counts); a kept row's position is that base + the kept rows of
//                            its image in the waves before it (LDS) + those in the lanes before it (ballot), so an
//                            image's rows keep their input order; rows past the counts are zeroed by the same launch.
// The integer LDS atomics of launch 0 only count, so every output is a pure function of the inputs.
namespace {

constexpr int REFINE_CHUNK = TDN_REFINE_CHUNK;
static_assert(REFINE_CHUNK == BLK, "one row per thread");

struct RefineArgs {
  const float* rois;          // (R, 5)
  const void* reg;            // (R, reg_cols)
  const int64_t* labels;      // (R,) or null
  const void* cls;            // (R, C) or null: the label is the arg-max, ties to the lowest column
  const int32_t* img_shapes;  // (B, 2)
  const int32_t* gt_inds;     // (R,) or null
  const float* gt;            // (B, G, 4) or null
  int32_t R, C, reg_cols, B, G, P;
  f32x4_t means, stds;
  float max_ratio;
};

// image of row r if the row is kept, else -1: padding, a class-specific label outside [0, C), or (compacted mode with
// gt_inds) a row whose four coordinates are bitwise those of its own ground truth
__device__ __forceinline__ int refine_image(const RefineArgs& A, int r, long long label) {
  int b = row_image(A.rois, IDX_ROI, r, A.B);
  if (A.reg_cols != 4 && (label < 0 || label >= A.C)) b = -1;
  if (b >= 0 && A.gt_inds) {
    const int gi = A.gt_inds[r];
    if (gi >= 0 && gi < A.G) {
      const uint32_t* p = (const uint32_t*)(A.rois + (size_t)r * 5 + 1);
      const uint32_t* g = (const uint32_t*)(A.gt + ((size_t)b * A.G + gi) * 4);
      if (p[0] == g[0] && p[1] == g[1] && p[2] == g[2] && p[3] == g[3]) b = -1;
    }
  }
  return b;
}

__global__ __launch_bounds__(BLK) void refine_count_kernel(const RefineArgs A, int* __restrict__ chunk_cnt) {
  __shared__ int cnt[64];
  const int tid = threadIdx.x;
  if (tid < 64) cnt[tid] = 0;
  __syncthreads();
  const int r = blockIdx.x * REFINE_CHUNK + tid;
  if (r < A.R) {
    // with class logits the arg-max is always inside [0, C): the label only matters when it is given
    const int b = refine_image(A, r, A.labels ? (long long)A.labels[r] : 0ll);
    if (b >= 0) atomicAdd(&cnt[b], 1);
  }
  __syncthreads();
  if (tid < A.B) chunk_cnt[blockIdx.x * A.B + tid] = cnt[tid];
}

// label of row r0 + lane: the wavefront takes its 64 rows ARGMAX_ROWS at a time (their loads are in flight together:
// one row after the other is a chain of 64 load latencies), lanes stride the columns
constexpr int ARGMAX_ROWS = 16;

template <class T>
__device__ __forceinline__ int wave_argmax(const T* cls, int r0, int R, int C, int lane) {
  int label = 0;
  for (int i0 = 0; i0 < 64 && r0 + i0 < R; i0 += ARGMAX_ROWS) {       // wave-uniform bounds
    // no branch around a load: a row past R reads row R - 1 (its label is never used), a lane past C column C - 1
    float best[ARGMAX_ROWS];
    int bi[ARGMAX_ROWS];
    const T* x[ARGMAX_ROWS];
#pragma unroll
    for (int k = 0; k < ARGMAX_ROWS; ++k) x[k] = cls + (size_t)min(r0 + i0 + k, R - 1) * C;
#pragma unroll
    for (int k = 0; k < ARGMAX_ROWS; ++k) {
      const float v = (float)x[k][min(lane, C - 1)];
      best[k] = lane < C ? v : -INFINITY;
      bi[k] = lane < C ? lane : 0x7fffffff;
    }
    for (int c = lane + 64; c < C; c += 64) {
      float v[ARGMAX_ROWS];
#pragma unroll
      for (int k = 0; k < ARGMAX_ROWS; ++k) v[k] = (float)x[k][c];
#pragma unroll
      for (int k = 0; k < ARGMAX_ROWS; ++k)
        if (v[k] > best[k]) {                         // ascending columns: the first of equals stays
          best[k] = v[k];
          bi[k] = c;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
      for (int k = 0; k < ARGMAX_ROWS; ++k) {
        const float ov = __shfl_xor(best[k], o);
        const int oi = __shfl_xor(bi[k], o);
        if (ov > best[k] || (ov == best[k] && oi < bi[k])) {
          best[k] = ov;
          bi[k] = oi;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < ARGMAX_ROWS; ++k)
      if (lane == i0 + k) label = bi[k];
  }
  return label;
}

template <int DT>
__device__ __forceinline__ f32x4_t refine_box(const RefineArgs& A, int r, int b, int label) {
  typedef typename DetElem<DT>::T T;
  const float* roi = A.rois + (size_t)r * 5;
  const f32x4_t rb = {roi[1], roi[2], roi[3], roi[4]};
  const T* dr = (const T*)A.reg + (size_t)r * A.reg_cols + (A.reg_cols == 4 ? 0 : 4 * label);
  f32x4_t d;
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = (float)dr[e];
  return decode_box(rb, d, A.means, A.stds, A.max_ratio, A.img_shapes[2 * b], A.img_shapes[2 * b + 1]);
}

template <int DT, bool COMPACT>
__global__ __launch_bounds__(BLK) void refine_kernel(const RefineArgs A, const int* __restrict__ chunk_cnt, int nchunks,
                                                     float* __restrict__ rois_out, float* __restrict__ props,
                                                     int32_t* __restrict__ counts) {
  typedef typename DetElem<DT>::T T;
  constexpr int W = BLK / 64;
  __shared__ int part[2][W][64];                      // [before this chunk | all chunks][slice][image]
  __shared__ int wcnt[W][64];                         // kept rows of (wave, image) in this chunk
  __shared__ int base[64], total[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (COMPACT) {
    int pre = 0, tot = 0;                             // thread (slice = wave, image = lane)
    if (lane < A.B)
      for (int c = wave; c < nchunks; c += W) {
        const int v = chunk_cnt[c * A.B + lane];
        tot += v;
        pre += c < (int)blockIdx.x ? v : 0;
      }
    part[0][wave][lane] = pre;
    part[1][wave][lane] = tot;
    wcnt[wave][lane] = 0;
    __syncthreads();
    if (tid < 64) {
      int p = 0, t = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        p += part[0][w][tid];
        t += part[1][w][tid];
      }
      base[tid] = p;
      total[tid] = t;
    }
    __syncthreads();
  }
  const int r = blockIdx.x * blockDim.x + tid;        // compacted: blockDim.x = REFINE_CHUNK
  const int r0 = r - lane;                            // the wavefront's first row
  long long label = 0;
  if (A.cls) label = wave_argmax((const T*)A.cls, r0, A.R, A.C, lane);
  else if (r < A.R) label = A.labels[r];
  const int b = r < A.R ? refine_image(A, r, label) : -1;
  const bool keep = b >= 0;
  if constexpr (!COMPACT) {
    if (r < A.R) {
      float* o = rois_out + (size_t)r * 5;
      f32x4_t bx = {0.f, 0.f, 0.f, 0.f};
      if (keep) bx = refine_box<DT>(A, r, b, (int)label);
      o[0] = keep ? (float)b : -1.f;
      o[1] = bx[0];
      o[2] = bx[1];
      o[3] = bx[2];
      o[4] = bx[3];
    }
  } else {
    // rank among the wavefront's kept rows of the same image: one ballot per distinct image of the wavefront
    const u64 below = (1ull << lane) - 1ull;
    int rank = 0;
    u64 todo = __ballot(keep);
    while (todo) {                                    // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int lb = __shfl(b, leader);
      const u64 same = __ballot(keep && b == lb);
      if (keep && b == lb) rank = __popcll(same & below);
      if (lane == leader) wcnt[wave][lb] = __popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    if (keep) {
      int pos = base[b] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][b];
      if (pos < A.P) {
        const f32x4_t bx = refine_box<DT>(A, r, b, (int)label);
        float* o = props + ((size_t)b * A.P + pos) * 5;
        o[0] = bx[0];
        o[1] = bx[1];
        o[2] = bx[2];
        o[3] = bx[3];
        o[4] = 0.f;
      }
    }
    // the rows past every image's count, shared out over the grid
    for (int q = blockIdx.x * BLK + tid; q < A.B * A.P; q += gridDim.x * BLK) {
      const int bq = q / A.P, p = q - bq * A.P;
      if (p >= total[bq]) {
        float* o = props + (size_t)q * 5;
#pragma unroll
        for (int e = 0; e < 5; ++e) o[e] = 0.f;
      }
    }
    if (blockIdx.x == 0 && tid < A.B) counts[tid] = min(total[tid], A.P);
  }
}

constexpr int REFINE_ROWS = 256;                      // rows per workgroup of the row-aligned launch (no LDS, no scan)

template <bool COMPACT>
void refine_launch(int dtype, dim3 grid, void* stream, const RefineArgs& A, const int* chunk_cnt, int nchunks,
                   float* rois_out, float* props, int32_t* counts) {
  const dim3 block(COMPACT ? BLK : REFINE_ROWS);
  if (dtype == TDN_F32) TDN_LAUNCH((refine_kernel<TDN_F32, COMPACT>), grid, block, 0, stream, A, chunk_cnt, nchunks, rois_out, props, counts);
  else if (dtype == TDN_BF16) TDN_LAUNCH((refine_kernel<TDN_BF16, COMPACT>), grid, block, 0, stream, A, chunk_cnt, nchunks, rois_out, props, counts);
  else TDN_LAUNCH((refine_kernel<TDN_F16, COMPACT>), grid, block, 0, stream, A, chunk_cnt, nchunks, rois_out, props, counts);
}

}  // namespace

extern "C" int tdn_refine_bboxes(const float* rois, const void* bbox_pred, int dtype, int R, int reg_cols, int B,
                                 const int32_t* img_shapes, const int64_t* labels, const void* cls_score, int C,
                                 const int32_t* pos_gt_inds, const float* gt_bboxes, int G, const float* means4,
                                 const float* stds4, double wh_ratio_clip, int max_per_img, float* rois_out,
                                 float* proposals, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  const char* who = "tdn_refine_bboxes";
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(dtype == TDN_F32 || dtype == TDN_BF16 || dtype == TDN_F16, "%s: dtype %d", who, dtype);
  TDN_CHECK(R >= 0 && R <= TDN_DET_MAX_ROWS, "%s: %d rows (max %d)", who, R, TDN_DET_MAX_ROWS);
  TDN_CHECK(C >= 1 && C <= TDN_DET_MAX_CLASSES, "%s: C=%d out of 1..%d", who, C, TDN_DET_MAX_CLASSES);
  TDN_CHECK(reg_cols == 4 || reg_cols == 4 * C, "%s: reg_cols=%d is neither 4 nor 4 * C", who, reg_cols);
  TDN_CHECK(max_per_img >= 0 && max_per_img <= TDN_RPN_MAX_NUM, "%s: max_per_img=%d out of 0..%d (0: row-aligned)", who,
            max_per_img, TDN_RPN_MAX_NUM);
  TDN_CHECK(means4 && stds4 && img_shapes, "%s: NULL means / stds / img_shapes", who);
  TDN_CHECK(wh_ratio_clip > 0.0 && wh_ratio_clip < 1.0, "%s: wh_ratio_clip must be in (0, 1)", who);
  TDN_CHECK((labels != nullptr) != (cls_score != nullptr) || R == 0, "%s: exactly one of labels and cls_score", who);
  TDN_CHECK(R == 0 || (rois && bbox_pred), "%s: NULL pointer", who);
  const bool compact = max_per_img > 0;
  TDN_CHECK(compact ? (proposals && counts) : (R == 0 || rois_out), "%s: NULL output", who);
  if (R == 0) pos_gt_inds = nullptr, gt_bboxes = nullptr;      // no row reads them
  TDN_CHECK((pos_gt_inds != nullptr) == (gt_bboxes != nullptr) && (!pos_gt_inds || (compact && G >= 1)),
            "%s: pos_gt_inds and gt_bboxes (B, G >= 1, 4) go together, in compacted mode only", who);
  RefineArgs A;
  memset(&A, 0, sizeof(A));
  A.rois = rois;
  A.reg = bbox_pred;
  A.labels = labels;
  A.cls = cls_score;
  A.img_shapes = img_shapes;
  A.gt_inds = pos_gt_inds;
  A.gt = gt_bboxes;
  A.R = R;
  A.C = C;
  A.reg_cols = reg_cols;
  A.B = B;
  A.G = G;
  A.P = max_per_img;
  A.means = host_f4(means4);
  A.stds = host_f4(stds4);
  A.max_ratio = (float)fabs(log(wh_ratio_clip));     // as tdn_delta2bbox: in double, rounded to fp32
  const int nchunks = (R + REFINE_CHUNK - 1) / REFINE_CHUNK;
  if (!compact) {
    if (R > 0) {
      refine_launch<false>(dtype, dim3((R + REFINE_ROWS - 1) / REFINE_ROWS), stream, A, nullptr, 0, rois_out, nullptr,
                           nullptr);
      TDN_LAUNCH_CHECK();
    }
    return 0;
  }
  int* chunk_cnt = nullptr;
  if (nchunks > 0) {
    tdn_carver c{(char*)workspace, 0};
    chunk_cnt = c.take<int>((int64_t)nchunks * B);
    if (tdn_check_ws(who, workspace, workspace_bytes, TDN_REFINE_WS_BYTES(R, B)) != 0) return -1;
    TDN_LAUNCH(refine_count_kernel, dim3(nchunks), dim3(BLK), 0, stream, A, chunk_cnt);
    TDN_LAUNCH_CHECK();
  }
  refine_launch<true>(dtype, dim3(nchunks > 0 ? nchunks : 1), stream, A, chunk_cnt, nchunks, nullptr, proposals, counts);
  TDN_LAUNCH_CHECK();
  return 0;
}

