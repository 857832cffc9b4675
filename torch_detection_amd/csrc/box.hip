// Box ops: anchor grid, pairwise IoU, greedy NMS.  HBM / latency-bound integer-index kernels.
//
// The reference has no implementation (core/__init__.py is empty); semantics are SURVEY.md Appendix B,
// consistent with the conventions the reference does pin: inclusive "+1" pixel boxes
// (datasets/utils/bbox.py:39,375-377), xyxy float32, x-fastest grid enumeration
// (datasets/dataset_transforms.py:120-131).  Arithmetic is strict IEEE fp32 in the oracle's operation
// order (this file is compiled with -ffp-contract=off; divisions are __fdiv_rn) so that results are
// bit-identical to oracle/box_ref.c.
#include "nms_core.h"
#include <string.h>

// ---- anchor grid -----------------------------------------------------------------------------------
__global__ void anchor_grid_kernel(const float* __restrict__ base, int A, int featH, int featW, int stride,
                                   int valid_h, int valid_w, float* __restrict__ anchors, uint8_t* valid) {
  const int total = featH * featW * A;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int a = i % A;
    const int cell = i / A;
    const int x = cell % featW, y = cell / featW;
    const float sx = (float)(x * stride), sy = (float)(y * stride);
    const f32x4_t b = *(const f32x4_t*)(base + a * 4);
    f32x4_t o;
    o[0] = b[0] + sx;
    o[1] = b[1] + sy;
    o[2] = b[2] + sx;
    o[3] = b[3] + sy;
    *(f32x4_t*)(anchors + (int64_t)i * 4) = o;
    if (valid) valid[i] = (x < valid_w && y < valid_h) ? 1 : 0;
  }
}

extern "C" int tdn_anchor_grid(const float* base_anchors, int A, int featH, int featW, int stride, int valid_h,
                               int valid_w, float* anchors, uint8_t* valid, void* stream) {
  TDN_CHECK(A > 0 && featH >= 0 && featW >= 0 && stride > 0, "tdn_anchor_grid: bad shape");
  const int64_t total = (int64_t)featH * featW * A;
  TDN_CHECK(total < (1ll << 30), "tdn_anchor_grid: too many anchors");
  if (total == 0) return 0;
  TDN_CHECK(base_anchors && anchors, "tdn_anchor_grid: NULL pointer");
  TDN_LAUNCH(anchor_grid_kernel, dim3(tdn_grid_1d(total, 256, 4096)), dim3(256), 0, (hipStream_t)stream, base_anchors, A,
             featH, featW, stride, valid_h, valid_w, anchors, valid);
  TDN_LAUNCH_CHECK();
  return 0;
}

// All levels of a pyramid in ONE launch (five launches of 4..70 us worth of work cost ~9 us each alone): level
// descriptors in the kernel-argument block, outputs concatenated level after level (order (y, x, anchor) inside a
// level, exactly as tdn_anchor_grid writes them).
constexpr int ANCHOR_MAXL = 8;
struct AnchorLevels {
  int nlevels, total;
  int start[ANCHOR_MAXL + 1];      // first anchor of level l; start[nlevels] = total
  int A[ANCHOR_MAXL], featW[ANCHOR_MAXL], stride[ANCHOR_MAXL], valid_h[ANCHOR_MAXL], valid_w[ANCHOR_MAXL];
  const float* base[ANCHOR_MAXL];
};

__global__ void anchor_pyramid_kernel(const AnchorLevels L, float* __restrict__ anchors, uint8_t* valid) {
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < L.total; g += gridDim.x * blockDim.x) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < ANCHOR_MAXL; ++k) l += (k < L.nlevels && g >= L.start[k]) ? 1 : 0;
    const int i = g - L.start[l];
    const int A = L.A[l], featW = L.featW[l], stride = L.stride[l];
    const int a = i % A;
    const int cell = i / A;
    const int x = cell % featW, y = cell / featW;
    const float sx = (float)(x * stride), sy = (float)(y * stride);
    const f32x4_t b = *(const f32x4_t*)(L.base[l] + a * 4);
    f32x4_t o;
    o[0] = b[0] + sx;
    o[1] = b[1] + sy;
    o[2] = b[2] + sx;
    o[3] = b[3] + sy;
    *(f32x4_t*)(anchors + (int64_t)g * 4) = o;
    if (valid) valid[g] = (x < L.valid_w[l] && y < L.valid_h[l]) ? 1 : 0;
  }
}

extern "C" int tdn_anchor_pyramid(const tdn_anchor_level* levels, int nlevels, float* anchors, uint8_t* valid,
                                  void* stream) {
  TDN_CHECK(levels != nullptr && nlevels > 0 && nlevels <= ANCHOR_MAXL, "tdn_anchor_pyramid: 1..%d levels",
            ANCHOR_MAXL);
  AnchorLevels L;
  memset(&L, 0, sizeof(L));
  L.nlevels = nlevels;
  int64_t total = 0;
  for (int l = 0; l < nlevels; ++l) {
    const tdn_anchor_level& s = levels[l];
    TDN_CHECK(s.A > 0 && s.featH >= 0 && s.featW >= 0 && s.stride > 0, "tdn_anchor_pyramid: level %d: bad shape", l);
    TDN_CHECK(s.base_anchors != nullptr, "tdn_anchor_pyramid: level %d: NULL base anchors", l);
    L.start[l] = (int)total;
    L.A[l] = s.A; L.featW[l] = s.featW > 0 ? s.featW : 1; L.stride[l] = s.stride;
    L.valid_h[l] = s.valid_h; L.valid_w[l] = s.valid_w; L.base[l] = s.base_anchors;
    total += (int64_t)s.featH * s.featW * s.A;
    TDN_CHECK(total < (1ll << 30), "tdn_anchor_pyramid: too many anchors");
  }
  for (int l = nlevels; l <= ANCHOR_MAXL; ++l) L.start[l] = (int)total;
  L.total = (int)total;
  if (total == 0) return 0;
  TDN_CHECK(anchors != nullptr, "tdn_anchor_pyramid: NULL output");
  TDN_LAUNCH(anchor_pyramid_kernel, dim3(tdn_grid_1d(total, 256, 4096)), dim3(256), 0, (hipStream_t)stream, L, anchors,
             valid);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- IoU -------------------------------------------------------------------------------------------
// A thread owns four consecutive columns (boxes of `b` and their areas stay in registers) and walks IOU_ROWS rows of
// `a` (workgroup-uniform: scalar loads): no index division, 16 B of `b` traffic per IOU_ROWS outputs, and a wave
// writes 1 KB of contiguous output per row.
constexpr int IOU_ROWS = 16;
__global__ __launch_bounds__(256) void iou_pairwise_kernel(const float* __restrict__ a, int N,
                                                           const float* __restrict__ b, int M,
                                                           float* __restrict__ out) {
  const int M4 = (M + 3) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;   // column quad
  if (q >= M4) return;
  const int j0 = q * 4;
  const bool vec_ok = (M & 3) == 0;
  f32x4_t bb[4];
  float ab[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = j0 + e;
    bb[e] = (j < M) ? *(const f32x4_t*)(b + (int64_t)j * 4) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
    ab[e] = box_area(bb[e]);
  }
  for (int ib = blockIdx.y * IOU_ROWS; ib < N; ib += gridDim.y * IOU_ROWS)
  for (int i = ib; i < min(N, ib + IOU_ROWS); ++i) {
    const f32x4_t ba = *(const f32x4_t*)(a + (int64_t)i * 4);
    const float area_a = box_area(ba);
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (j0 + e < M) ? box_iou2(ba, area_a, bb[e], ab[e]) : 0.f;
    float* o = out + (int64_t)i * M + j0;
    if (vec_ok) {
      *(f32x4_t*)o = (f32x4_t){r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j0 + e < M) o[e] = r[e];
    }
  }
}

extern "C" int tdn_bbox_iou_pairwise(const float* a, int N, const float* b, int M, float* iou, void* stream) {
  TDN_CHECK(N >= 0 && M >= 0, "tdn_bbox_iou_pairwise: negative size");
  if (N == 0 || M == 0) return 0;
  TDN_CHECK(a && b && iou, "tdn_bbox_iou_pairwise: NULL pointer");
  const int M4 = (M + 3) / 4;
  int gy = (N + IOU_ROWS - 1) / IOU_ROWS;
  if (gy > 65535) gy = 65535;   // the kernel strides over row blocks
  TDN_LAUNCH(iou_pairwise_kernel, dim3((M4 + 255) / 256, gy), dim3(256), 0, (hipStream_t)stream, a, N, b, M, iou);
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- NMS -------------------------------------------------------------------------------------------
// (1) rank[i] = #{ j : s[j] > s[i]  or  (s[j] == s[i] and j < i) }  -> stable descending order.
__global__ void nms_rank_kernel(const float* __restrict__ scores, int N, int jchunk, int* rank) {
  __shared__ float sj[1024];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const float si = (i < N) ? scores[i] : 0.f;
  const int jb = blockIdx.y * jchunk, je = min(N, jb + jchunk);
  int cnt = 0;
  for (int base = jb; base < je; base += 1024) {
    const int n = min(1024, je - base);
    for (int k = threadIdx.x; k < n; k += blockDim.x) sj[k] = scores[base + k];
    __syncthreads();
    if (i < N) {
      for (int k = 0; k < n; ++k) {
        const float s = sj[k];
        const int j = base + k;
        cnt += (s > si || (s == si && j < i)) ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (i < N && cnt) atomicAdd(&rank[i], cnt);
}

__global__ void nms_scatter_kernel(const float* __restrict__ boxes, const int* __restrict__ rank, int N, int* order,
                                   float* sboxes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int r = rank[i];
  order[r] = i;
  *(f32x4_t*)(sboxes + (int64_t)r * 4) = *(const f32x4_t*)(boxes + (int64_t)i * 4);
}

// (2) 64-bit suppression words: mask[i][cb] bit b  <=>  j = cb*64+b > i  and  iou(i, j) > thr   (sorted order);
//     one wave per 64 x 64 block (nms_core.h).
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ sboxes, int N, float thr, int nblk,
                                                      unsigned long long* __restrict__ mask) {
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;
  nms_mask_block(sboxes, N, thr, nblk, rb, cb, mask);
}

// (3) serial keep scan by ONE wave: 64-box chunks; within a chunk the diagonal words are resolved with
//     readlane + bit ops, then the kept rows are OR-ed into the running removal bitmap (lane = word).
__global__ __launch_bounds__(64) void nms_scan_kernel(const unsigned long long* __restrict__ mask,
                                                      const int* __restrict__ order, int N, int nblk,
                                                      uint8_t* keep, int64_t* kept_idx, int* num_kept) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long remv[];  // [nblk] removal bitmap
  const int lane = threadIdx.x;
  for (int w = lane; w < nblk; w += 64) remv[w] = 0ull;
  __syncthreads();
  int cnt = 0;
  for (int c = 0; c < nblk; ++c) {
    const int i = c * 64 + lane;
    const unsigned long long diag = (i < N) ? mask[(int64_t)i * nblk + c] : 0ull;
    const int nvalid = min(64, N - c * 64);
    unsigned long long alive = ~remv[c];
    if (nvalid < 64) alive &= (1ull << nvalid) - 1ull;
    unsigned long long keepbits = 0ull;
    const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
    while (alive) {
      const int b = __builtin_ctzll(alive);
      keepbits |= 1ull << b;
      alive &= ~(1ull << b);
      const unsigned lo = __builtin_amdgcn_readlane(dlo, b), hi = __builtin_amdgcn_readlane(dhi, b);
      alive &= ~(((unsigned long long)hi << 32) | lo);
    }
    // outputs for this chunk
    if (i < N) {
      const bool k = (keepbits >> lane) & 1ull;
      const int oi = order[i];
      keep[oi] = k ? 1 : 0;
      if (k) {
        const int pos = cnt + __builtin_popcountll(keepbits & ((1ull << lane) - 1ull));
        kept_idx[pos] = (int64_t)oi;
      }
    }
    cnt += __builtin_popcountll(keepbits);
    // OR kept rows into remv for the remaining words; lane handles words c+1+lane, +64, ...
    for (int w = c + 1 + lane; w < nblk; w += 64) {
      unsigned long long acc = 0ull;
      unsigned long long kb = keepbits;
      while (kb) {
        // up to 4 independent row loads in flight
        int b0 = __builtin_ctzll(kb); kb &= kb - 1;
        unsigned long long v0 = mask[(int64_t)(c * 64 + b0) * nblk + w], v1 = 0, v2 = 0, v3 = 0;
        if (kb) { int b1 = __builtin_ctzll(kb); kb &= kb - 1; v1 = mask[(int64_t)(c * 64 + b1) * nblk + w]; }
        if (kb) { int b2 = __builtin_ctzll(kb); kb &= kb - 1; v2 = mask[(int64_t)(c * 64 + b2) * nblk + w]; }
        if (kb) { int b3 = __builtin_ctzll(kb); kb &= kb - 1; v3 = mask[(int64_t)(c * 64 + b3) * nblk + w]; }
        acc |= (v0 | v1) | (v2 | v3);
      }
      remv[w] |= acc;
    }
    __syncthreads();  // single wave: orders this chunk's remv writes before the next chunk's read
  }
  for (int k = cnt + lane; k < N; k += 64) kept_idx[k] = -1;
  if (lane == 0) *num_kept = cnt;
}

// (3') the same scan by a 1024-thread workgroup, in super-chunks of 1024 boxes, serial part in LDS (nms_core.h).
__global__ __launch_bounds__(1024) void nms_scan_block_kernel(const unsigned long long* __restrict__ mask,
                                                              const int* __restrict__ order, int N, int nblk,
                                                              uint8_t* keep, int64_t* kept_idx, int* num_kept) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sm[];
  nms_scan_block(mask, order, N, nblk, nblk, keep, kept_idx, num_kept, sm);
}

struct NmsWs { int *rank, *order; float* sboxes; unsigned long long* mask; int64_t bytes; };
static NmsWs nms_layout(int N, void* base) {   // N >= 1; a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<int>(N), c.take<int>(N), c.take<float>(4ll * N),
          c.take<unsigned long long>((int64_t)N * ((N + 63) / 64)), c.off + 256};   // one spare block, as ever
}
extern "C" int64_t tdn_nms_workspace(int N) { return N <= 0 ? 256 : nms_layout(N, nullptr).bytes; }

extern "C" int tdn_nms(const float* boxes, const float* scores, int N, float iou_thr, uint8_t* keep,
                       int64_t* kept_idx, int32_t* num_kept, void* workspace, int64_t workspace_bytes,
                       void* stream) {
  hipStream_t st = (hipStream_t)stream;
  TDN_CHECK(N >= 0 && N <= 64 * 8000, "tdn_nms: N=%d out of range (0..512000)", N);
  TDN_CHECK(num_kept != nullptr, "tdn_nms: NULL num_kept");
  if (N == 0) {
    TDN_MEMSET_ASYNC(num_kept, 0, sizeof(int32_t), st);
    return 0;
  }
  TDN_CHECK(boxes && scores && keep && kept_idx && workspace, "tdn_nms: NULL pointer");
  const NmsWs w = nms_layout(N, workspace);
  if (tdn_check_ws("tdn_nms", workspace, workspace_bytes, w.bytes) != 0) return -1;
  const int nblk = (N + 63) / 64;
  TDN_MEMSET_ASYNC(w.rank, 0, (size_t)N * 4, st);
  const int nb = (N + 255) / 256;
  int jsplit = 1024 / nb;  // aim for ~1024 blocks
  if (jsplit < 1) jsplit = 1;
  if (jsplit > (N + 1023) / 1024) jsplit = (N + 1023) / 1024;
  const int jchunk = ((N + jsplit - 1) / jsplit + 1023) / 1024 * 1024;
  jsplit = (N + jchunk - 1) / jchunk;
  TDN_LAUNCH(nms_rank_kernel, dim3(nb, jsplit), dim3(256), 0, st, scores, N, jchunk, w.rank);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(nms_scatter_kernel, dim3(nb), dim3(256), 0, st, boxes, (const int*)w.rank, N, w.order, w.sboxes);
  TDN_LAUNCH_CHECK();
  TDN_LAUNCH(nms_mask_kernel, dim3(nblk, nblk), dim3(64), 0, st, (const float*)w.sboxes, N, iou_thr, nblk, w.mask);
  TDN_LAUNCH_CHECK();
  const char* ow = tdn_knob_present("TDN_NMS_ONEWAVE");
  const bool one_wave = ow && ow[0] == '1';   // A/B runs
  if (nblk <= NMS_BLOCK_MAX_NBLK && !one_wave) {
    const size_t lds = nms_scan_block_lds(nblk);
    if (tdn_allow_lds<nms_scan_block_kernel>(160 * 1024, "nms_scan_block") < 0) return -1;
    TDN_LAUNCH(nms_scan_block_kernel, dim3(1), dim3(1024), lds, st, (const unsigned long long*)w.mask,
               (const int*)w.order, N, nblk, keep, kept_idx, num_kept);
  } else {
    TDN_LAUNCH(nms_scan_kernel, dim3(1), dim3(64), (size_t)nblk * 8, st, (const unsigned long long*)w.mask,
               (const int*)w.order, N, nblk, keep, kept_idx, num_kept);
  }
  TDN_LAUNCH_CHECK();
  return 0;
}

// ---- box delta (de)normalisation: datasets/utils/bbox.py:118-166 of the reference --------------------------
// normalize: bbox <- (bbox - means) / stds, IN PLACE like the reference (bbox.sub_(means).div_(stds), bbox.py:140);
// denormalize: out = bbox * stds + means with means/stds tiled over the 4C columns (bbox.py:161-165).
// Separate IEEE sub/div and mul/add (no FMA) so results are bit-identical to the PyTorch-CPU reference.
__global__ void bbox_normalize_kernel(float* bbox, int64_t n4, f32x4_t means, f32x4_t stds) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4_t v = *(f32x4_t*)(bbox + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __fdiv_rn(__fsub_rn(v[e], means[e]), stds[e]);
    *(f32x4_t*)(bbox + i * 4) = v;
  }
}

__global__ void bbox_denormalize_kernel(const float* __restrict__ bbox, float* __restrict__ out, int64_t n4,
                                        f32x4_t means, f32x4_t stds) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4_t v = *(const f32x4_t*)(bbox + i * 4);
    f32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __fadd_rn(__fmul_rn(v[e], stds[e]), means[e]);
    *(f32x4_t*)(out + i * 4) = o;
  }
}

extern "C" int tdn_bbox_normalize(float* bbox, int64_t rows, const float* means4, const float* stds4, void* stream) {
  TDN_CHECK(rows >= 0 && means4 && stds4, "tdn_bbox_normalize: bad arguments");
  if (rows == 0) return 0;
  TDN_CHECK(bbox != nullptr, "tdn_bbox_normalize: NULL bbox");
  const f32x4_t m = host_f4(means4), s = host_f4(stds4);   // by value: a recorded launch must not keep the pointers
  TDN_LAUNCH(bbox_normalize_kernel, dim3(tdn_grid_1d(rows, 256, 4096)), dim3(256), 0, (hipStream_t)stream, bbox, rows,
             m, s);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_bbox_denormalize(const float* bbox, float* out, int64_t rows, int cols, const float* means4,
                                    const float* stds4, void* stream) {
  TDN_CHECK(rows >= 0 && cols > 0 && cols % 4 == 0 && means4 && stds4, "tdn_bbox_denormalize: cols must be 4C");
  const int64_t n4 = rows * (cols / 4);
  if (n4 == 0) return 0;
  TDN_CHECK(bbox && out, "tdn_bbox_denormalize: NULL pointer");
  const f32x4_t m = host_f4(means4), s = host_f4(stds4);
  TDN_LAUNCH(bbox_denormalize_kernel, dim3(tdn_grid_1d(n4, 256, 4096)), dim3(256), 0, (hipStream_t)stream, bbox, out,
             n4, m, s);
  TDN_LAUNCH_CHECK();
  return 0;
}
