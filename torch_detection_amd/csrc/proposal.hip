// Box delta encode / decode, segmented greedy NMS and the fused RPN proposal pipeline.
//
// Semantics are the project's own spec in the mmdetection-v0.x lineage of SURVEY Appendix B ('+1' boxes, strict IEEE
// fp32 in the spec's operation order: this file is compiled with -ffp-contract=off, products and sums are __f*_rn);
// the CPU restatement is tests/proposal_ref.py.
//
// rpn_proposals is four launches for any B and L:
//   1 rpn_topk_decode_kernel  one workgroup per (image, level) segment: radix select of the nms_pre highest logits
//                             (11/11/10-bit digits over an order-preserving 32-bit key, LDS histograms), an ordered
//                             compaction (ties at the threshold key lowest anchor first), an LDS bitonic sort of the
//                             composite keys (key << 32 | ~anchor), then per selected row: anchor + delta gather,
//                             decode, clip, min-size filter, ordered compaction into the segment's rows.
//   2 nms_mask_seg_kernel     suppression words of every segment: grid (column block, row block, segment).
//   3 nms_scan_seg_kernel     the 1024-thread keep scan of box.hip, one workgroup per segment.  The rows of a segment
//                             already are in key order, so no ranking step.
//   4 rpn_merge_kernel        one workgroup per image: select + sort the best max_num of the levels' first nms_post
//                             survivors by (logit desc, concatenated anchor index asc), write the padded outputs.
// batched_nms is a sort kernel (one workgroup per segment: bitonic sort of (score key, ~row)) + launches 2 and 3.
// Nothing here uses a float atomic or waits on another workgroup; the integer LDS atomics only count, so every
// output is a pure function of the inputs.
#include "nms_core.h"
#include "select_core.h"
#include "delta_core.h"
#include <math.h>
#include <string.h>

__device__ __forceinline__ float load_elem(const void* p, int dtype, int64_t off) {
  if (dtype == TDN_F32) return ((const float*)p)[off];
  return __uint_as_float((uint32_t)((const uint16_t*)p)[off] << 16);   // bf16 -> fp32 is exact
}

__global__ void bbox2delta_kernel(const float* __restrict__ prop, const float* __restrict__ gt, int64_t N,
                                  f32x4_t means, f32x4_t stds, float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
    *(f32x4_t*)(out + i * 4) = encode_box(*(const f32x4_t*)(prop + i * 4), *(const f32x4_t*)(gt + i * 4), means, stds);
}

__global__ void delta2bbox_kernel(const float* __restrict__ rois, const float* __restrict__ deltas, int64_t N, int C,
                                  f32x4_t means, f32x4_t stds, float max_ratio, int clip_h, int clip_w,
                                  float* __restrict__ out) {
  const int64_t total = N * C;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = q / C;
    *(f32x4_t*)(out + q * 4) = decode_box(*(const f32x4_t*)(rois + row * 4), *(const f32x4_t*)(deltas + q * 4), means,
                                          stds, max_ratio, clip_h, clip_w);
  }
}

extern "C" int tdn_bbox2delta(const float* proposals, const float* gt, int64_t N, const float* means4,
                              const float* stds4, float* deltas, void* stream) {
  TDN_CHECK(N >= 0 && means4 && stds4, "tdn_bbox2delta: bad arguments");
  if (N == 0) return 0;
  TDN_CHECK(proposals && gt && deltas, "tdn_bbox2delta: NULL pointer");
  TDN_LAUNCH(bbox2delta_kernel, dim3(tdn_grid_1d(N, 256, 4096)), dim3(256), 0, (hipStream_t)stream, proposals, gt, N,
             host_f4(means4), host_f4(stds4), deltas);
  TDN_LAUNCH_CHECK();
  return 0;
}

// |log(wh_ratio_clip)| evaluated in double, rounded to fp32 (16/1000 -> 4.1351666f)
static float max_ratio_of(double wh_ratio_clip) { return (float)fabs(log(wh_ratio_clip)); }

extern "C" int tdn_delta2bbox(const float* rois, const float* deltas, int64_t N, int C, const float* means4,
                              const float* stds4, const int32_t* max_shape, double wh_ratio_clip, float* out,
                              void* stream) {
  TDN_CHECK(N >= 0 && C > 0 && means4 && stds4, "tdn_delta2bbox: bad arguments");
  TDN_CHECK(wh_ratio_clip > 0.0 && wh_ratio_clip < 1.0, "tdn_delta2bbox: wh_ratio_clip must be in (0, 1)");
  TDN_CHECK(!max_shape || (max_shape[0] > 0 && max_shape[1] > 0), "tdn_delta2bbox: bad max_shape");
  if (N == 0) return 0;
  TDN_CHECK(rois && deltas && out, "tdn_delta2bbox: NULL pointer");
  TDN_LAUNCH(delta2bbox_kernel, dim3(tdn_grid_1d(N * C, 256, 4096)), dim3(256), 0, (hipStream_t)stream, rois, deltas, N,
             C, host_f4(means4), host_f4(stds4), max_ratio_of(wh_ratio_clip), max_shape ? max_shape[0] : -1,
             max_shape ? max_shape[1] : -1, out);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- RPN proposals ----------------------------------------------------------------------------------------------
struct RpnArgs {
  int L, per_img, nms_post, max_num, pitch;
  float min_size, max_ratio;
  f32x4_t means, stds;
  const void* logits[TDN_RPN_MAX_LEVELS];
  const void* deltas[TDN_RPN_MAX_LEVELS];
  const float* anchors[TDN_RPN_MAX_LEVELS];
  int64_t ls[TDN_RPN_MAX_LEVELS][4], ds[TDN_RPN_MAX_LEVELS][4];
  int dtype[TDN_RPN_MAX_LEVELS], W[TDN_RPN_MAX_LEVELS], A[TDN_RPN_MAX_LEVELS];
  int n[TDN_RPN_MAX_LEVELS], cap[TDN_RPN_MAX_LEVELS], cap_off[TDN_RPN_MAX_LEVELS], aoff[TDN_RPN_MAX_LEVELS];
};

// logit keys of one (image, level): anchor i = (y*W + x)*A + a -> element (b, a, y, x) through the strides
struct LogitFetch {
  const void* p;
  int64_t base, sc, sh, sw;
  int dtype, A, W;
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
    int a = i0 % A;
    const int cell = i0 / A;
    int y = cell / W, x = cell - (cell / W) * W;
#pragma unroll
    for (int e = 0; e < TK_PER; ++e) {
      if (e < cnt) kk[e] = order_key(load_elem(p, dtype, base + a * sc + y * sh + x * sw));
      if (++a == A) {
        a = 0;
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    }
  }
};

constexpr int RPN_SEG_MAX = TDN_NMS_SEG_MAX;
constexpr size_t TOPK_LDS = (size_t)RPN_SEG_MAX * 8 + TK_BINS * 4 + TK_MISC * 4;               // 41.2 KB
constexpr size_t MERGE_LDS = (size_t)TDN_RPN_MAX_NUM * 8 + TK_BINS * 4 + TK_MISC * 4;          // 72.3 KB

__global__ __launch_bounds__(1024) void rpn_topk_decode_kernel(const RpnArgs P, const int32_t* __restrict__ img_shapes,
                                                               f32x4_t* seg_box, uint32_t* seg_key, int* seg_aidx,
                                                               int* seg_start, int* seg_count) {
  extern __shared__ __attribute__((aligned(16))) u64 smem[];
  u64* skeys = smem;                                  // [RPN_SEG_MAX]
  int* hist = (int*)(smem + RPN_SEG_MAX);             // [TK_BINS]
  int* misc = hist + TK_BINS;                         // [TK_MISC]
  const int tid = threadIdx.x;
  const int s = blockIdx.x, b = s / P.L, l = s - (s / P.L) * P.L;
  const int n = P.n[l], A = P.A[l], W = P.W[l];
  const int start = b * P.per_img + P.cap_off[l];
  const LogitFetch F{P.logits[l], b * P.ls[l][0], P.ls[l][1], P.ls[l][2], P.ls[l][3], P.dtype[l], A, W};
  const int m = block_topk(F, n, P.cap[l], skeys, hist, misc);
  // decode the selected rows in key order; a thread takes `per` consecutive rows, so one scan keeps the order
  const int ih = img_shapes[2 * b], iw = img_shapes[2 * b + 1];
  const int per = (m + BLK - 1) / BLK;                // <= 4
  const int64_t* ds = P.ds[l];
  f32x4_t box[RPN_SEG_MAX / BLK];
  uint32_t key[RPN_SEG_MAX / BLK];
  int idx[RPN_SEG_MAX / BLK];
  int ok = 0;
#pragma unroll
  for (int e = 0; e < RPN_SEG_MAX / BLK; ++e) {
    const int p = tid * per + e;
    key[e] = 0u;
    idx[e] = -1;
    if (e < per && p < m) {
      const u64 c = skeys[p];
      key[e] = (uint32_t)(c >> 32);
      const int i = (int)~(uint32_t)c;
      const int a = i % A, cell = i / A, y = cell / W, x = cell - (cell / W) * W;
      const int64_t o = b * ds[0] + y * ds[2] + x * ds[3] + (int64_t)(4 * a) * ds[1];
      f32x4_t d;
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = load_elem(P.deltas[l], P.dtype[l], o + j * ds[1]);
      box[e] = decode_box(*(const f32x4_t*)(P.anchors[l] + (int64_t)i * 4), d, P.means, P.stds, P.max_ratio, ih, iw);
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
  int total;
  int q = start + block_excl_scan(ok, misc, &total);
#pragma unroll
  for (int e = 0; e < RPN_SEG_MAX / BLK; ++e)
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

// one workgroup per segment: rows [seg_start, +seg_count) of sboxes, mask rows of `pitch` words
__global__ __launch_bounds__(64) void nms_mask_seg_kernel(const float* __restrict__ sboxes, const int* seg_start,
                                                          const int* seg_count, float thr, int pitch,
                                                          unsigned long long* __restrict__ mask) {
  const int s = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;
  const int n = seg_count[s];
  if (cb * 64 >= n) return;                           // also n <= 0; rb <= cb
  const int64_t start = seg_start[s];
  nms_mask_block(sboxes + start * 4, n, thr, pitch, rb, cb, mask + start * pitch);
}

// kept_idx[start + r]: kept rows (order == nullptr: segment-local row, else order[start + row]); num_kept[s] = count,
// -1 for a segment marked invalid (seg_count < 0)
__global__ __launch_bounds__(1024) void nms_scan_seg_kernel(const unsigned long long* __restrict__ mask,
                                                            const int* __restrict__ order, const int* seg_start,
                                                            const int* seg_count, int pitch, uint8_t* keep,
                                                            int64_t* kept_idx, int* num_kept) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sm[];
  const int s = blockIdx.x;
  const int n = seg_count[s];
  if (n <= 0) {
    if (threadIdx.x == 0) num_kept[s] = n < 0 ? -1 : 0;
    return;
  }
  const int64_t start = seg_start[s];
  nms_scan_block(mask + start * pitch, order ? order + start : nullptr, n, (n + 63) / 64, pitch, keep,
                 kept_idx + start, num_kept + s, sm);
}

// candidates of one image: the first min(num_kept, nms_post) survivors of each level, level after level
struct MergeFetch {
  const int* cum;           // [L + 1] LDS
  const int* st;            // [L] LDS: segment starts
  int L;
  const int64_t* kept;
  const uint32_t* seg_key;
  __device__ __forceinline__ int row(int j) const {
    int l = 0;
    while (l + 1 < L && j >= cum[l + 1]) ++l;
    return st[l] + (int)kept[st[l] + j - cum[l]];
  }
  __device__ __forceinline__ void operator()(int i0, int cnt, uint32_t* kk) const {
#pragma unroll
    for (int e = 0; e < TK_PER; ++e)
      if (e < cnt) kk[e] = seg_key[row(i0 + e)];
  }
};

__global__ __launch_bounds__(1024) void rpn_merge_kernel(const RpnArgs P, const f32x4_t* __restrict__ seg_box,
                                                         const uint32_t* __restrict__ seg_key,
                                                         const int* __restrict__ seg_aidx, const int* seg_start,
                                                         const int64_t* __restrict__ kept, const int* num_kept,
                                                         float* proposals, int64_t* anchor_idx, int32_t* counts) {
  extern __shared__ __attribute__((aligned(16))) u64 smem[];
  u64* skeys = smem;                                  // [TDN_RPN_MAX_NUM]
  int* hist = (int*)(smem + TDN_RPN_MAX_NUM);         // [TK_BINS]
  int* misc = hist + TK_BINS;                         // [TK_MISC]
  int* cum = misc + 32;                               // [L + 1]
  int* st = cum + TDN_RPN_MAX_LEVELS + 1;             // [L]
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid == 0) {
    int c = 0;
    for (int l = 0; l < P.L; ++l) {
      const int s = b * P.L + l;
      cum[l] = c;
      st[l] = seg_start[s];
      c += min(num_kept[s], P.nms_post);
    }
    cum[P.L] = c;
  }
  __syncthreads();
  const MergeFetch F{cum, st, P.L, kept, seg_key};
  const int T = cum[P.L];
  const int m = block_topk(F, T, min(P.max_num, T), skeys, hist, misc);
  for (int p = tid; p < P.max_num; p += BLK) {
    float* o = proposals + ((int64_t)b * P.max_num + p) * 5;
    int64_t* ai = anchor_idx + (int64_t)b * P.max_num + p;
    if (p < m) {
      const u64 c = skeys[p];
      const int r = F.row((int)~(uint32_t)c);
      const f32x4_t bx = seg_box[r];
      const float logit = key_value((uint32_t)(c >> 32));
      o[0] = bx[0];
      o[1] = bx[1];
      o[2] = bx[2];
      o[3] = bx[3];
      o[4] = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-logit)));
      *ai = seg_aidx[r];
    } else {
#pragma unroll
      for (int e = 0; e < 5; ++e) o[e] = 0.f;
      *ai = -1;
    }
  }
  if (tid == 0) counts[b] = m;
}

struct RpnPlan {
  RpnArgs P;
  int B, S, maxcap;
  int64_t rows;
};

static int rpn_plan(const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg, RpnPlan* out) {
  TDN_CHECK(levels && cfg, "tdn_rpn_proposals: NULL levels / config");
  TDN_CHECK(nlevels >= 1 && nlevels <= TDN_RPN_MAX_LEVELS, "tdn_rpn_proposals: 1..%d levels", TDN_RPN_MAX_LEVELS);
  if (tdn_check_batch("tdn_rpn_proposals", B) != 0) return -1;
  TDN_CHECK(cfg->nms_pre >= 0 && cfg->nms_post >= 1 && cfg->max_num >= 1 && cfg->max_num <= TDN_RPN_MAX_NUM,
            "tdn_rpn_proposals: bad nms_pre / nms_post / max_num");
  TDN_CHECK(cfg->min_bbox_size >= 0.f && cfg->nms_thr == cfg->nms_thr, "tdn_rpn_proposals: bad min_bbox_size / nms_thr");
  RpnArgs& P = out->P;
  memset(&P, 0, sizeof(P));
  P.L = nlevels;
  P.nms_post = cfg->nms_post;
  P.max_num = cfg->max_num;
  P.min_size = cfg->min_bbox_size;
  P.max_ratio = max_ratio_of(16.0 / 1000.0);
  P.means = host_f4(cfg->means);
  P.stds = host_f4(cfg->stds);
  int64_t per_img = 0, aoff = 0;
  int maxcap = 0;
  for (int l = 0; l < nlevels; ++l) {
    const tdn_rpn_level& v = levels[l];
    TDN_CHECK(v.dtype == TDN_F32 || v.dtype == TDN_BF16, "tdn_rpn_proposals: level %d: dtype must be TDN_F32 or TDN_BF16", l);
    TDN_CHECK(v.H >= 0 && v.W >= 0 && v.A >= 1, "tdn_rpn_proposals: level %d: bad H / W / A", l);
    const int64_t n = (int64_t)v.H * v.W * v.A;
    TDN_CHECK(n == 0 || (v.logits && v.deltas && v.anchors), "tdn_rpn_proposals: level %d: NULL pointer", l);
    const int64_t cap = cfg->nms_pre > 0 ? (n < cfg->nms_pre ? n : cfg->nms_pre) : n;
    TDN_CHECK(cap <= RPN_SEG_MAX, "tdn_rpn_proposals: level %d sends %lld boxes to NMS (max %d)", l, (long long)cap,
              RPN_SEG_MAX);
    for (int e = 0; e < 4; ++e)
      TDN_CHECK(v.logit_strides[e] >= 0 && v.delta_strides[e] >= 0, "tdn_rpn_proposals: level %d: negative stride", l);
    P.logits[l] = v.logits;
    P.deltas[l] = v.deltas;
    P.anchors[l] = v.anchors;
    memcpy(P.ls[l], v.logit_strides, sizeof(P.ls[l]));
    memcpy(P.ds[l], v.delta_strides, sizeof(P.ds[l]));
    P.dtype[l] = v.dtype;
    P.W[l] = v.W > 0 ? v.W : 1;
    P.A[l] = v.A;
    P.n[l] = (int)n;
    P.cap[l] = (int)cap;
    P.cap_off[l] = (int)per_img;
    P.aoff[l] = (int)aoff;
    per_img += cap;
    aoff += n;
    TDN_CHECK(aoff < (1ll << 30), "tdn_rpn_proposals: too many anchors");
    if (cap > maxcap) maxcap = (int)cap;
  }
  P.per_img = (int)per_img;
  P.pitch = maxcap > 0 ? (maxcap + 63) / 64 : 1;
  out->B = B;
  out->S = B * nlevels;
  out->maxcap = maxcap;
  out->rows = per_img * B;
  return 0;
}

struct RpnWs {
  f32x4_t* seg_box; uint32_t* seg_key; int* seg_aidx; int64_t* kept;
  int *seg_start, *seg_count, *num_kept; u64* mask; int64_t bytes;
};
static RpnWs rpn_layout(const RpnPlan& p, void* base) {   // a braced list is evaluated left to right
  const int64_t R = p.rows > 0 ? p.rows : 1;   // every level empty: one placeholder row
  tdn_carver c{(char*)base, 0};
  return {c.take<f32x4_t>(R), c.take<uint32_t>(R), c.take<int>(R), c.take<int64_t>(R),
          c.take<int>(p.S), c.take<int>(p.S), c.take<int>(p.S), c.take<u64>(R * p.P.pitch), c.off};
}

extern "C" int64_t tdn_rpn_proposals_workspace(const tdn_rpn_level* levels, int nlevels, int B,
                                               const tdn_rpn_config* cfg) {
  RpnPlan p;
  if (rpn_plan(levels, nlevels, B, cfg, &p) != 0) return -1;
  return rpn_layout(p, nullptr).bytes;
}

extern "C" int tdn_rpn_proposals(const tdn_rpn_level* levels, int nlevels, int B, const int32_t* img_shapes,
                                 const tdn_rpn_config* cfg, float* proposals, int64_t* anchor_idx, int32_t* counts,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  RpnPlan p;
  if (rpn_plan(levels, nlevels, B, cfg, &p) != 0) return -1;
  TDN_CHECK(img_shapes && proposals && anchor_idx && counts && workspace, "tdn_rpn_proposals: NULL pointer");
  const RpnWs w = rpn_layout(p, workspace);
  if (tdn_check_ws("tdn_rpn_proposals", workspace, workspace_bytes, w.bytes) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int pitch = p.P.pitch;
  TDN_LAUNCH(rpn_topk_decode_kernel, dim3(p.S), dim3(BLK), TOPK_LDS, st, p.P, img_shapes, w.seg_box, w.seg_key,
             w.seg_aidx, w.seg_start, w.seg_count);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(nms_mask_seg_kernel, dim3(pitch, pitch, p.S), dim3(64), 0, st, (const float*)w.seg_box,
             (const int*)w.seg_start, (const int*)w.seg_count, cfg->nms_thr, pitch, w.mask);
  TDN_LAUNCH_CHECK();
  if (tdn_allow_lds<nms_scan_seg_kernel>(160 * 1024, "nms_scan_seg") < 0) return -1;
  TDN_LAUNCH(nms_scan_seg_kernel, dim3(p.S), dim3(BLK), nms_scan_block_lds(pitch), st,
             (const unsigned long long*)w.mask, (const int*)nullptr, (const int*)w.seg_start, (const int*)w.seg_count,
             pitch, (uint8_t*)nullptr, w.kept, w.num_kept);
  TDN_LAUNCH_CHECK();
  if (tdn_allow_lds<rpn_merge_kernel>(160 * 1024, "rpn_merge") < 0) return -1;
  TDN_LAUNCH(rpn_merge_kernel, dim3(p.B), dim3(BLK), MERGE_LDS, st, p.P, (const f32x4_t*)w.seg_box,
             (const uint32_t*)w.seg_key, (const int*)w.seg_aidx, (const int*)w.seg_start, (const int64_t*)w.kept,
             (const int*)w.num_kept, proposals, anchor_idx, counts);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- hooks for guided.hip (proposal_host.h): the workspace and launches 2-4 on their own --------------------------
#include "proposal_host.h"

int tdn_rpn_ws_layout(const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg, void* base,
                      tdn_rpn_ws* out) {
  RpnPlan p;
  if (rpn_plan(levels, nlevels, B, cfg, &p) != 0) return -1;
  const RpnWs w = rpn_layout(p, base);
  *out = {w.seg_box, w.seg_key, w.seg_aidx, w.kept, w.seg_start, w.seg_count, w.num_kept, w.mask, w.bytes};
  return 0;
}

int tdn_rpn_nms_merge(const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg, const tdn_rpn_ws* w,
                      float* proposals, int64_t* anchor_idx, int32_t* counts, void* stream) {
  RpnPlan p;
  if (rpn_plan(levels, nlevels, B, cfg, &p) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int pitch = p.P.pitch;
  TDN_LAUNCH(nms_mask_seg_kernel, dim3(pitch, pitch, p.S), dim3(64), 0, st, (const float*)w->seg_box,
             (const int*)w->seg_start, (const int*)w->seg_count, cfg->nms_thr, pitch, w->mask);
  TDN_LAUNCH_CHECK();
  if (tdn_allow_lds<nms_scan_seg_kernel>(160 * 1024, "nms_scan_seg") < 0) return -1;
  TDN_LAUNCH(nms_scan_seg_kernel, dim3(p.S), dim3(BLK), nms_scan_block_lds(pitch), st,
             (const unsigned long long*)w->mask, (const int*)nullptr, (const int*)w->seg_start, (const int*)w->seg_count,
             pitch, (uint8_t*)nullptr, w->kept, w->num_kept);
  TDN_LAUNCH_CHECK();
  if (tdn_allow_lds<rpn_merge_kernel>(160 * 1024, "rpn_merge") < 0) return -1;
  TDN_LAUNCH(rpn_merge_kernel, dim3(p.B), dim3(BLK), MERGE_LDS, st, p.P, (const f32x4_t*)w->seg_box,
             (const uint32_t*)w->seg_key, (const int*)w->seg_aidx, (const int*)w->seg_start, (const int64_t*)w->kept,
             (const int*)w->num_kept, proposals, anchor_idx, counts);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- batched NMS ------------------------------------------------------------------------------------------------
// one workgroup per segment: (score key, ~row) sorted descending -> order (input index) and the boxes in that order
__global__ __launch_bounds__(1024) void nms_seg_sort_kernel(const float* __restrict__ boxes,
                                                            const float* __restrict__ scores, int N,
                                                            const int64_t* __restrict__ seg_offsets, int* order,
                                                            float* sboxes, int* seg_start, int* seg_count) {
  extern __shared__ __attribute__((aligned(16))) u64 skeys[];   // [TDN_NMS_SEG_MAX]
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t a = seg_offsets[s], e = seg_offsets[s + 1];
  if (!(a >= 0 && a <= e && e <= N && e - a <= TDN_NMS_SEG_MAX)) {
    if (tid == 0) {
      seg_start[s] = 0;
      seg_count[s] = -1;
    }
    return;
  }
  const int n = (int)(e - a);
  const int P = pow2_ceil(n);
  for (int i = tid; i < P; i += BLK) skeys[i] = i < n ? compose(order_key(scores[a + i]), i) : 0ull;
  block_sort_desc(skeys, P);
  for (int p = tid; p < n; p += BLK) {
    const int i = (int)~(uint32_t)skeys[p];
    order[a + p] = (int)a + i;
    *(f32x4_t*)(sboxes + (a + p) * 4) = *(const f32x4_t*)(boxes + (a + i) * 4);
  }
  if (tid == 0) {
    seg_start[s] = (int)a;
    seg_count[s] = n;
  }
}

static int nms_seg_pitch(int N) {
  const int m = N < TDN_NMS_SEG_MAX ? N : TDN_NMS_SEG_MAX;
  return m > 0 ? (m + 63) / 64 : 1;
}

struct SegNmsWs { int* order; float* sboxes; int *seg_start, *seg_count; u64* mask; int64_t bytes; };
static SegNmsWs seg_nms_layout(int N, int S, void* base) {
  const int64_t n = N > 0 ? N : 1, s = S > 0 ? S : 1;   // placeholders: no region is empty
  tdn_carver c{(char*)base, 0};
  return {c.take<int>(n), c.take<float>(n * 4), c.take<int>(s), c.take<int>(s), c.take<u64>(n * nms_seg_pitch(N)),
          c.off};
}
extern "C" int64_t tdn_batched_nms_workspace(int N, int S) {
  return (N < 0 || S < 0) ? -1 : seg_nms_layout(N, S, nullptr).bytes;
}

extern "C" int tdn_batched_nms(const float* boxes, const float* scores, int N, const int64_t* seg_offsets, int S,
                               float iou_thr, uint8_t* keep, int64_t* kept_idx, int32_t* counts, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TDN_CHECK(N >= 0 && N < (1 << 30) && S >= 0 && S < (1 << 24), "tdn_batched_nms: bad N / S");
  if (N > 0) {
    TDN_CHECK(keep && kept_idx, "tdn_batched_nms: NULL keep / kept_idx");
    TDN_MEMSET_ASYNC(keep, 0, (size_t)N, st);
    TDN_MEMSET_ASYNC(kept_idx, 0xFF, (size_t)N * 8, st);             // -1
  }
  if (S == 0) return 0;
  TDN_CHECK(seg_offsets && counts && workspace && (N == 0 || (boxes && scores)), "tdn_batched_nms: NULL pointer");
  const SegNmsWs w = seg_nms_layout(N, S, workspace);
  if (tdn_check_ws("tdn_batched_nms", workspace, workspace_bytes, w.bytes) != 0) return -1;
  const int pitch = nms_seg_pitch(N);
  TDN_LAUNCH(nms_seg_sort_kernel, dim3(S), dim3(BLK), (size_t)TDN_NMS_SEG_MAX * 8, st, boxes, scores, N, seg_offsets,
             w.order, w.sboxes, w.seg_start, w.seg_count);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(nms_mask_seg_kernel, dim3(pitch, pitch, S), dim3(64), 0, st, (const float*)w.sboxes,
             (const int*)w.seg_start, (const int*)w.seg_count, iou_thr, pitch, w.mask);
  TDN_LAUNCH_CHECK();
  if (tdn_allow_lds<nms_scan_seg_kernel>(160 * 1024, "nms_scan_seg") < 0) return -1;
  TDN_LAUNCH(nms_scan_seg_kernel, dim3(S), dim3(BLK), nms_scan_block_lds(pitch), st, (const unsigned long long*)w.mask,
             (const int*)w.order, (const int*)w.seg_start, (const int*)w.seg_count, pitch, keep, kept_idx, counts);
  TDN_LAUNCH_CHECK();
  return 0;
}
