// Single-stage (RetinaNet-style) dense anchor heads: test-time detections from sigmoid class logits, and unsampled,
// class-labelled anchor targets.
//
// Semantics are the project's own spec in the mmdetection-v1 lineage (AnchorHead.get_bboxes, anchor_target with
// sampling off), '+1' boxes, strict IEEE fp32 in the spec's operation order (this file is compiled with
// -ffp-contract=off); the CPU restatement is tests/dense_detect_ref.py.
//
// tdn_dense_detections is seven launches for any B, number of levels and C:
//   1 dd_key_kernel            the class maximum of every anchor of the levels that select (n_l > nms_pre > 0), as an
//                              order-preserving 32-bit key; the grid grows with the anchors.  Logits whose pixels'
//                              A*C channels are contiguous (channels_last) are staged through LDS with 16-byte loads
//                              and reduced one anchor per thread from rows of odd pitch; any other layout is read
//                              through its strides, pixel-fastest, one anchor per thread.
//   2 dd_select_decode_kernel  one workgroup per (image, level): radix threshold of the nms_pre-th key
//                              (select_core.h), ordered compaction of the kept anchors in ANCHOR order, then per kept
//                              row the decode (delta_core.h), the background column, batch_idx, anchor_idx, and per
//                              (row, class) the sigmoid: the dense tensors, each element written once.
//   3-6                        tdn_multiclass_nms (detect.hip) on the dense tensors; tdn_dense_detections_soft:
//                              tdn_multiclass_nms_soft there, three launches.
//   7 dd_anchor_gather_kernel  anchor_idx[b][j] = dense_anchor_idx[row_idx[b][j]], -1 on unused rows.
// tdn_anchor_target_all is the assignment launches of tdn_anchor_target (target.hip, through target_host.h) plus
//   dd_target_fill_kernel      labels, weights, encode and the per-image counts: one returning 64-bit integer atomic add
//                              per workgroup packs (positives, negatives, workgroups done); the workgroup that comes last
//                              reads the totals off its own add and writes num_pos / num_neg.
// No memset, no float atomics, no inter-workgroup waits, no allocation; integer atomics only count, so every output is a
// pure function of the inputs.
#include "select_core.h"
#include "delta_core.h"
#include "target_host.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int DD_SEG_MAX = TDN_NMS_SEG_MAX;
constexpr int KEY_THREADS = 256;
constexpr int KEY_TILE = 8192;                 // floats of LDS per workgroup of the key kernel (32 KB)
constexpr int KEY_INFLIGHT = 4;               // 16-byte loads a thread of the key kernel keeps in flight

struct DdLevel {
  const void* cls;
  const void* reg;
  const float* anchors;
  int64_t cs[4], rs[4];
  int H, W;
  int n, k;                                    // anchors, anchors kept
  int koff, aoff, keyoff;                      // prefix sums of k, of n, of n rounded up to 4 (key words)
  int blk_end, nblk, ta;                       // key launch: end of the level's workgroups, per image, anchors in each
  int fast;                                    // a pixel's A*C logits and the pixels of an image are contiguous
};

struct DdArgs {
  int L, B, A, C, K, N, NK, dtype;             // K = sum k, N = sum n, NK = key words per image
  float max_ratio, scale;
  f32x4_t means, stds;
  const int32_t* img_shapes;
  const float* scales;
  DdLevel lv[TDN_DENSE_MAX_LEVELS];
};

__device__ __forceinline__ float dd_load(const void* p, int dtype, int64_t off) {
  if (dtype == TDN_F32) return ((const float*)p)[off];
  if (dtype == TDN_F16) return (float)((const f16_t*)p)[off];
  return __uint_as_float((uint32_t)((const uint16_t*)p)[off] << 16);   // bf16 -> fp32 is exact
}

// ---- 1: class maximum of every anchor ------------------------------------------------------------------------------
// the 4 or 8 elements of one 16-byte vector, element e first, widened into the tile's rows of pitch Cp
__device__ __forceinline__ void key_scatter(const uint4 raw, int dtype, int e, int C, int Cp, float* tile) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  float x[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (dtype == TDN_F32) {
      x[j] = __uint_as_float(w[j]);
      x[4 + j] = 0.f;
    } else if (dtype == TDN_F16) {
      x[2 * j] = (float)__builtin_bit_cast(f16_t, (uint16_t)(w[j] & 0xFFFFu));
      x[2 * j + 1] = (float)__builtin_bit_cast(f16_t, (uint16_t)(w[j] >> 16));
    } else {
      x[2 * j] = __uint_as_float(w[j] << 16);
      x[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
    }
  }
  const int nel = dtype == TDN_F32 ? 4 : 8;
  int a = e / C, c = e - a * C;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < nel) {
      tile[a * Cp + c] = x[j];
      if (++c == C) {
        c = 0;
        ++a;
      }
    }
}

__global__ __launch_bounds__(KEY_THREADS) void dd_key_kernel(const DdArgs P, uint32_t* __restrict__ keys) {
  __shared__ __attribute__((aligned(16))) float tile[KEY_TILE];
  const int tid = threadIdx.x, blk = blockIdx.x;
  int l = 0;
  while (l + 1 < P.L && blk >= P.lv[l].blk_end) ++l;
  const DdLevel& V = P.lv[l];
  const int r = blk - (V.blk_end - P.B * V.nblk);
  const int b = r / V.nblk, a0 = (r - b * V.nblk) * V.ta;
  const int na = min(V.ta, V.n - a0), C = P.C, dtype = P.dtype;
  uint32_t* out = keys + (int64_t)b * P.NK + V.keyoff;
  if (V.fast) {
    // anchor i's classes are elements [i*C, (i+1)*C) of the image's block: the tile is ne contiguous elements
    const int Cp = C | 1;                      // odd pitch: the per-anchor reads below touch 32 different banks
    const int ne = na * C;
    const int64_t base = b * V.cs[0] + (int64_t)a0 * C;
    const int esz = dtype == TDN_F32 ? 4 : 2, VEC = 16 / esz;
    const char* src = (const char*)V.cls + base * esz;
    if (((uintptr_t)src & 15) == 0) {
      // the whole 16-byte vectors, KEY_INFLIGHT loads of a thread issued before the first is used; then the tail
      const int nv = ne / VEC;
      for (int v0 = tid; v0 < nv; v0 += KEY_THREADS * KEY_INFLIGHT) {
        uint4 raw[KEY_INFLIGHT];
#pragma unroll
        for (int u = 0; u < KEY_INFLIGHT; ++u) {
          const int v = v0 + u * KEY_THREADS;
          if (v < nv) raw[u] = *(const uint4*)(src + (int64_t)v * 16);
        }
#pragma unroll
        for (int u = 0; u < KEY_INFLIGHT; ++u) {
          const int v = v0 + u * KEY_THREADS;
          if (v < nv) key_scatter(raw[u], dtype, v * VEC, C, Cp, tile);
        }
      }
      for (int e = nv * VEC + tid; e < ne; e += KEY_THREADS) {
        const int a = e / C;
        tile[a * Cp + (e - a * C)] = dd_load(V.cls, dtype, base + e);
      }
    } else {
      for (int e = tid; e < ne; e += KEY_THREADS) {
        const int a = e / C;
        tile[a * Cp + (e - a * C)] = dd_load(V.cls, dtype, base + e);
      }
    }
    __syncthreads();
    if (tid < na) {
      const float* row = tile + tid * Cp;
      float m = row[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
      out[a0 + tid] = order_key(m);
    }
    return;
  }
  // any other layout: item t = a * H*W + pixel, so that the lanes of a wavefront walk the pixels of one channel
  const int t = a0 + tid;
  if (t >= V.n) return;
  const int HW = V.H * V.W;
  const int a = t / HW, p = t - a * HW, y = p / V.W, x = p - y * V.W;
  const int64_t off = b * V.cs[0] + (int64_t)a * C * V.cs[1] + y * V.cs[2] + x * V.cs[3];
  float m = dd_load(V.cls, dtype, off);
  for (int c = 1; c < C; ++c) m = fmaxf(m, dd_load(V.cls, dtype, off + c * V.cs[1]));
  out[p * P.A + a] = order_key(m);
}

// ---- 2: per (image, level) selection, decode and sigmoid -----------------------------------------------------------
// keys of one (image, level): contiguous words from a 16-byte boundary
struct KeyFetch {
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

__global__ __launch_bounds__(BLK) void dd_select_decode_kernel(const DdArgs P, const uint32_t* __restrict__ keys,
                                                               float* __restrict__ scores, float* __restrict__ boxes,
                                                               int32_t* __restrict__ bidx, int64_t* __restrict__ aidx) {
  __shared__ int hist[TK_BINS];
  __shared__ int misc[TK_MISC];
  __shared__ int sel[DD_SEG_MAX];              // the kept anchors of a level that selects, ascending
  const int tid = threadIdx.x;
  const int s = blockIdx.x, b = s / P.L, l = s - b * P.L;
  const DdLevel& V = P.lv[l];
  const int n = V.n, k = V.k, C = P.C, A = P.A, W = V.W, dtype = P.dtype;
  const bool selecting = n > k;
  if (selecting) {
    const KeyFetch F{keys + (int64_t)b * P.NK + V.keyoff};
    int need;
    const uint32_t T = block_radix_threshold(F, n, k, hist, misc, &need);
    // keys > T and the first `need` keys == T, in anchor order: a thread takes TK_PER consecutive anchors, so one scan
    // of both counts (packed: a step holds at most 8192 of either) places a whole step
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
          ng += kk[e] > T ? 1 : 0;
          nt += kk[e] == T ? 1 : 0;
        }
      int tot;
      const int ex = block_excl_scan(ng | (nt << 16), misc, &tot);
      int tb = ties_done + (ex >> 16);                            // ties before this thread's first anchor
      int pos = gt_done + (ex & 0xFFFF) + min(tb, need);          // kept anchors before it
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) {
          if (kk[e] > T) {
            sel[pos++] = i0 + e;
          } else if (kk[e] == T) {
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
  const bool rescale = P.scales || P.scale != 0.f;
  const float sc = P.scales ? P.scales[b] : P.scale;
  // one thread per kept row: decode, background column, batch_idx, anchor_idx
  for (int r = tid; r < k; r += BLK) {
    const int i = selecting ? sel[r] : r;
    const int a = i % A, cell = i / A, y = cell / W, x = cell - y * W;
    const int64_t o = b * V.rs[0] + y * V.rs[2] + x * V.rs[3] + (int64_t)(4 * a) * V.rs[1];
    f32x4_t d;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = dd_load(V.reg, dtype, o + j * V.rs[1]);
    f32x4_t bx = decode_box(*(const f32x4_t*)(V.anchors + (int64_t)i * 4), d, P.means, P.stds, P.max_ratio, ih, iw);
    if (rescale) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bx[e] = __fdiv_rn(bx[e], sc);
    }
    *(f32x4_t*)(boxes + (row0 + r) * 4) = bx;
    scores[(row0 + r) * (C + 1)] = 0.f;
    bidx[row0 + r] = b;
    aidx[row0 + r] = (int64_t)V.aoff + i;
  }
  // one thread per (kept row, class), class fastest: the rows' stores are contiguous, and so are channels_last loads
  const int64_t total = (int64_t)k * C;
  for (int64_t q = tid; q < total; q += BLK) {
    const int r = (int)(q / C), c = (int)(q - (int64_t)r * C);
    const int i = selecting ? sel[r] : r;
    const int a = i % A, cell = i / A, y = cell / W, x = cell - y * W;
    const float v = dd_load(V.cls, dtype, b * V.cs[0] + ((int64_t)a * C + c) * V.cs[1] + y * V.cs[2] + x * V.cs[3]);
    scores[(row0 + r) * (C + 1) + 1 + c] = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-v)));
  }
}

// ---- 7: the pyramid anchor of every detection ------------------------------------------------------------------------
__global__ void dd_anchor_gather_kernel(const int64_t* __restrict__ row_idx, const int64_t* __restrict__ dense_aidx,
                                        int n, int64_t* __restrict__ anchor_idx) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) {
    const int64_t r = row_idx[q];
    anchor_idx[q] = r >= 0 ? dense_aidx[r] : -1;
  }
}

// ---- unsampled anchor targets: every output element and the counts -----------------------------------------------
constexpr int FILL_THREADS = 256;
constexpr int FILL_MAX_BLOCKS = 2048;          // per image: the count word has 22 bits for them
constexpr int CNT_BITS = 21;                   // positives, negatives <= TDN_TARGET_MAX_BOXES = 2^20

struct FillAllArgs {
  const float* anchors;
  int64_t stride;
  const float* gt;
  const int64_t* gt_labels;
  int N, G;
  f32x4_t means, stds;
};

__global__ __launch_bounds__(FILL_THREADS) void dd_target_fill_kernel(const FillAllArgs A,
                                                                      const int32_t* __restrict__ assigned,
                                                                      int64_t* __restrict__ labels,
                                                                      float* __restrict__ label_weights,
                                                                      float* __restrict__ bbox_targets,
                                                                      float* __restrict__ bbox_weights, u64* cnt,
                                                                      int32_t* num_pos, int32_t* num_neg) {
  __shared__ int part[2 * FILL_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  int np = 0, nn = 0;
  for (int i = blockIdx.x * FILL_THREADS + tid; i < A.N; i += gridDim.x * FILL_THREADS) {
    const int64_t q = (int64_t)b * A.N + i;
    const int a = assigned[q];
    f32x4_t t = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    int64_t lab = 0;
    if (a > 0) {
      const int64_t gi = (int64_t)b * A.G + a - 1;
      const f32x4_t bx = *(const f32x4_t*)(A.anchors + b * A.stride + (int64_t)i * 4);
      t = encode_box(bx, *(const f32x4_t*)(A.gt + gi * 4), A.means, A.stds);
      w = (f32x4_t){1.f, 1.f, 1.f, 1.f};
      lab = A.gt_labels ? A.gt_labels[gi] : 1;
    }
    labels[q] = lab;
    label_weights[q] = a >= 0 ? 1.f : 0.f;
    *(f32x4_t*)(bbox_targets + q * 4) = t;
    *(f32x4_t*)(bbox_weights + q * 4) = w;
    np += a > 0 ? 1 : 0;
    nn += a == 0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    np += __shfl_xor(np, o);
    nn += __shfl_xor(nn, o);
  }
  if ((tid & 63) == 0) {
    part[2 * (tid >> 6)] = np;
    part[2 * (tid >> 6) + 1] = nn;
  }
  __syncthreads();
  if (tid == 0) {
    u64 add = 1ull << (2 * CNT_BITS);
    for (int w = 0; w < FILL_THREADS / 64; ++w) add += (u64)part[2 * w] | ((u64)part[2 * w + 1] << CNT_BITS);
    const u64 now = atomicAdd(cnt + b, add) + add;               // everything this image has counted so far
    if ((int)(now >> (2 * CNT_BITS)) == (int)gridDim.x) {        // this workgroup came last
      num_pos[b] = (int32_t)(now & ((1ull << CNT_BITS) - 1));
      num_neg[b] = (int32_t)((now >> CNT_BITS) & ((1ull << CNT_BITS) - 1));
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct DdPlan {
  DdArgs A;
  int key_blocks, selecting;
  int64_t rows;                                // B * K
  int64_t nms_bytes;
};

// the checks and the geometry the plan query, the workspace query and the call share; pointers may be null
int dd_plan(const char* who, const tdn_dense_level* levels, int L, int B, const tdn_dense_config* cfg, DdPlan* out, bool soft = false) {
  TDN_CHECK(levels && cfg, "%s: NULL levels / config", who);
  TDN_CHECK(L >= 1 && L <= TDN_DENSE_MAX_LEVELS, "%s: %d levels (1..%d)", who, L, TDN_DENSE_MAX_LEVELS);
  if (tdn_check_batch(who, B) != 0) return -1;
  const int A = cfg->num_anchors, C = cfg->num_classes;
  TDN_CHECK(cfg->dtype == TDN_F32 || cfg->dtype == TDN_BF16 || cfg->dtype == TDN_F16, "%s: dtype %d", who, cfg->dtype);
  TDN_CHECK(C >= 1 && C <= TDN_DET_MAX_CLASSES - 1, "%s: C=%d out of 1..%d", who, C, TDN_DET_MAX_CLASSES - 1);
  TDN_CHECK(A >= 1, "%s: A=%d anchors per pixel", who, A);
  TDN_CHECK(cfg->nms_pre >= 0 && cfg->nms_pre <= DD_SEG_MAX, "%s: nms_pre=%d out of 0..%d", who, cfg->nms_pre,
            DD_SEG_MAX);
  TDN_CHECK(cfg->max_num >= 1 && cfg->max_num <= TDN_RPN_MAX_NUM, "%s: max_num=%d out of 1..%d", who, cfg->max_num,
            TDN_RPN_MAX_NUM);
  TDN_CHECK(cfg->score_thr - cfg->score_thr == 0.f && (soft || cfg->nms_thr - cfg->nms_thr == 0.f),
            "%s: score_thr / nms_thr must be finite", who);
  TDN_CHECK(cfg->wh_ratio_clip > 0.0 && cfg->wh_ratio_clip < 1.0, "%s: wh_ratio_clip must be in (0, 1)", who);
  memset(out, 0, sizeof(*out));
  DdArgs& P = out->A;
  P.L = L;
  P.B = B;
  P.A = A;
  P.C = C;
  P.dtype = cfg->dtype;
  const int Cp = C | 1;
  int64_t K = 0, N = 0, NK = 0, blocks = 0;
  for (int l = 0; l < L; ++l) {
    const tdn_dense_level& v = levels[l];
    DdLevel& V = P.lv[l];
    TDN_CHECK(v.H >= 1 && v.W >= 1, "%s: level %d is %d x %d", who, l, v.H, v.W);
    const int64_t elems = (int64_t)B * A * C * v.H * v.W;
    TDN_CHECK(elems < (1ll << 31), "%s: level %d holds %lld logits (2^31 or more)", who, l, (long long)elems);
    const int64_t n = (int64_t)v.H * v.W * A;
    V.cls = v.cls;
    V.reg = v.reg;
    V.anchors = v.anchors;
    memcpy(V.cs, v.cls_strides, sizeof(V.cs));
    memcpy(V.rs, v.reg_strides, sizeof(V.rs));
    V.H = v.H;
    V.W = v.W;
    V.n = (int)n;
    V.k = (cfg->nms_pre > 0 && n > cfg->nms_pre) ? cfg->nms_pre : (int)n;
    TDN_CHECK(K + V.k <= TDN_DET_MAX_ROWS && N + n < (1ll << 31), "%s: more than %d dense rows", who,
              TDN_DET_MAX_ROWS);
    V.koff = (int)K;
    V.aoff = (int)N;
    V.keyoff = (int)NK;
    V.fast = v.cls_strides[1] == 1 && v.cls_strides[3] == (int64_t)A * C &&
             (v.H == 1 || v.cls_strides[2] == (int64_t)v.W * A * C);
    V.ta = V.fast ? (KEY_TILE / Cp < KEY_THREADS ? KEY_TILE / Cp : KEY_THREADS) : KEY_THREADS;
    V.nblk = V.n > V.k ? (V.n + V.ta - 1) / V.ta : 0;
    blocks += (int64_t)B * V.nblk;
    TDN_CHECK(blocks < (1ll << 31), "%s: too many workgroups", who);
    V.blk_end = (int)blocks;
    out->selecting += V.n > V.k;
    K += V.k;
    N += n;
    NK += (n + 3) & ~3ll;
  }
  out->rows = (int64_t)B * K;
  TDN_CHECK(out->rows <= TDN_DET_MAX_ROWS, "%s: B * K = %lld dense rows (max %d)", who, (long long)out->rows,
            TDN_DET_MAX_ROWS);
  const int64_t seg = (int64_t)B * C * (out->rows < DD_SEG_MAX ? out->rows : DD_SEG_MAX);
  TDN_CHECK(seg < (1ll << 31), "%s: B * C * min(B * K, %d) segment rows do not fit 31 bits", who, DD_SEG_MAX);
  P.K = (int)K;
  P.N = (int)N;
  P.NK = (int)NK;
  out->key_blocks = (int)blocks;
  P.max_ratio = (float)fabs(log(cfg->wh_ratio_clip));   // as tdn_delta2bbox: in double, rounded to fp32
  P.means = host_f4(cfg->means);
  P.stds = host_f4(cfg->stds);
  out->nms_bytes = soft ? tdn_multiclass_nms_soft_workspace_bytes((int)out->rows, C + 1, B)
                        : tdn_multiclass_nms_workspace_bytes((int)out->rows, C + 1, B);
  return out->nms_bytes < 0 ? -1 : 0;
}

struct DdWs { uint32_t* keys; char* nms; int64_t bytes; };
DdWs dd_layout(const DdPlan& p, void* base) {   // a braced list is evaluated left to right
  tdn_carver c{(char*)base, 0};
  return {c.take<uint32_t>(p.selecting ? (int64_t)p.A.B * p.A.NK : 0), c.take<char>(p.nms_bytes), c.off};
}

}  // namespace

extern "C" int tdn_dense_detections_plan(const tdn_dense_level* levels, int nlevels, int B,
                                         const tdn_dense_config* cfg, int32_t* out16) {
  DdPlan p;
  if (dd_plan("tdn_dense_detections_plan", levels, nlevels, B, cfg, &p) != 0) return -1;
  TDN_CHECK(out16, "tdn_dense_detections_plan: NULL output");
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

extern "C" int64_t tdn_dense_detections_workspace_bytes(const tdn_dense_level* levels, int nlevels, int B,
                                                        const tdn_dense_config* cfg) {
  DdPlan p;
  if (dd_plan("tdn_dense_detections", levels, nlevels, B, cfg, &p) != 0) return -1;
  return dd_layout(p, nullptr).bytes;
}

extern "C" int64_t tdn_dense_detections_soft_workspace_bytes(const tdn_dense_level* levels, int nlevels, int B,
                                                             const tdn_dense_config* cfg) {
  DdPlan p;
  if (dd_plan("tdn_dense_detections_soft", levels, nlevels, B, cfg, &p, true) != 0) return -1;
  return dd_layout(p, nullptr).bytes;
}

namespace {
// tdn_dense_detections (soft == null) and tdn_dense_detections_soft
int dd_run(const char* who, const tdn_dense_level* levels, int nlevels, int B, const int32_t* img_shapes,
           const float* scale_factors, const tdn_dense_config* cfg, const tdn_soft_nms_config* soft, float* dense_scores,
           float* dense_boxes, int32_t* batch_idx, int64_t* dense_anchor_idx, float* dets, int64_t* labels,
           int64_t* row_idx, int64_t* anchor_idx, int32_t* counts, void* workspace, int64_t workspace_bytes,
           void* stream) {
  DdPlan p;
  if (dd_plan(who, levels, nlevels, B, cfg, &p, soft != nullptr) != 0) return -1;
  TDN_CHECK(scale_factors || cfg->scale_factor == 0.f ||
                (cfg->scale_factor > 0.f && cfg->scale_factor - cfg->scale_factor == 0.f),
            "%s: scale_factor must be positive and finite (0: none)", who);
  TDN_CHECK(img_shapes && dense_scores && dense_boxes && batch_idx && dense_anchor_idx && dets && labels && row_idx &&
                anchor_idx && counts, "%s: NULL pointer", who);
  for (int l = 0; l < nlevels; ++l)
    TDN_CHECK(levels[l].cls && levels[l].reg && levels[l].anchors, "%s: level %d has a NULL pointer", who, l);
  const DdWs w = dd_layout(p, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  DdArgs& P = p.A;
  P.img_shapes = img_shapes;
  P.scales = scale_factors;
  P.scale = scale_factors ? 0.f : cfg->scale_factor;
  hipStream_t st = (hipStream_t)stream;
  if (p.key_blocks > 0) {
    TDN_LAUNCH(dd_key_kernel, dim3(p.key_blocks), dim3(KEY_THREADS), 0, st, P, w.keys);
    TDN_LAUNCH_CHECK();
  }
  TDN_LAUNCH(dd_select_decode_kernel, dim3(B * nlevels), dim3(BLK), 0, st, P, (const uint32_t*)w.keys, dense_scores,
             dense_boxes, batch_idx, dense_anchor_idx);
  TDN_LAUNCH_CHECK();
  const int rc = soft ? tdn_multiclass_nms_soft(dense_boxes, 4, dense_scores, batch_idx, 4, (int)p.rows, P.C + 1, B,
                                                cfg->score_thr, soft, cfg->max_num, dets, labels, row_idx, counts, w.nms,
                                                p.nms_bytes, stream)
                      : tdn_multiclass_nms(dense_boxes, 4, dense_scores, batch_idx, 4, (int)p.rows, P.C + 1, B,
                                           cfg->score_thr, cfg->nms_thr, cfg->max_num, dets, labels, row_idx, counts,
                                           w.nms, p.nms_bytes, stream);
  if (rc != 0) return rc;
  const int nd = B * cfg->max_num;
  TDN_LAUNCH(dd_anchor_gather_kernel, dim3((nd + 255) / 256), dim3(256), 0, st, (const int64_t*)row_idx,
             (const int64_t*)dense_anchor_idx, nd, anchor_idx);
  TDN_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int tdn_dense_detections(const tdn_dense_level* levels, int nlevels, int B, const int32_t* img_shapes,
                                    const float* scale_factors, const tdn_dense_config* cfg, float* dense_scores,
                                    float* dense_boxes, int32_t* batch_idx, int64_t* dense_anchor_idx, float* dets,
                                    int64_t* labels, int64_t* row_idx, int64_t* anchor_idx, int32_t* counts,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  return dd_run("tdn_dense_detections", levels, nlevels, B, img_shapes, scale_factors, cfg, nullptr, dense_scores,
                dense_boxes, batch_idx, dense_anchor_idx, dets, labels, row_idx, anchor_idx, counts, workspace,
                workspace_bytes, stream);
}

extern "C" int tdn_dense_detections_soft(const tdn_dense_level* levels, int nlevels, int B, const int32_t* img_shapes,
                                         const float* scale_factors, const tdn_dense_config* cfg,
                                         const tdn_soft_nms_config* soft, float* dense_scores, float* dense_boxes,
                                         int32_t* batch_idx, int64_t* dense_anchor_idx, float* dets, int64_t* labels,
                                         int64_t* row_idx, int64_t* anchor_idx, int32_t* counts, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_dense_detections_soft";
  if (tdn_soft_nms_check(who, soft) != 0) return -1;  // before the first launch
  return dd_run(who, levels, nlevels, B, img_shapes, scale_factors, cfg, soft, dense_scores, dense_boxes, batch_idx,
                dense_anchor_idx, dets, labels, row_idx, anchor_idx, counts, workspace, workspace_bytes, stream);
}

extern "C" int64_t tdn_anchor_target_all_workspace_bytes(int B, int N, int G) {
  const char* who = "tdn_anchor_target_all_workspace_bytes";
  if (tdn_check_batch(who, B) != 0) return -1;
  TDN_CHECK(N >= 1 && N <= TDN_TARGET_MAX_BOXES, "%s: %d boxes per image (1..%d)", who, N, TDN_TARGET_MAX_BOXES);
  TDN_CHECK(G >= 0 && G <= TDN_TARGET_MAX_GT, "%s: G=%d ground truths per image (max %d)", who, G, TDN_TARGET_MAX_GT);
  return tdn_target_anchor_assign_bytes(B, G, 2 * (int64_t)B);
}

extern "C" int tdn_anchor_target_all(const float* anchors, int64_t box_stride, const uint8_t* valid,
                                     int64_t valid_stride, const float* gt, const int64_t* gt_labels,
                                     const int32_t* gt_counts, const int32_t* img_shapes, int B, int N, int G,
                                     const tdn_target_config* cfg, int64_t* labels, float* label_weights,
                                     float* bbox_targets, float* bbox_weights, int32_t* num_pos, int32_t* num_neg,
                                     int32_t* assigned, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "tdn_anchor_target_all";
  const int64_t need = tdn_anchor_target_all_workspace_bytes(B, N, G);
  if (need < 0) return -1;
  TDN_CHECK(labels && label_weights && bbox_targets && bbox_weights && num_pos && num_neg, "%s: NULL output", who);
  if (tdn_check_ws(who, workspace, workspace_bytes, need) != 0) return -1;
  uint32_t* extra = nullptr;
  const int rc = tdn_target_anchor_assign(who, anchors, box_stride, valid, valid_stride, gt, gt_counts, img_shapes, B, N,
                                          G, cfg, assigned, workspace, 2 * (int64_t)B, &extra, stream);
  if (rc != 0) return rc;
  FillAllArgs F;
  F.anchors = anchors;
  F.stride = box_stride;
  F.gt = gt;
  F.gt_labels = G > 0 ? gt_labels : nullptr;
  F.N = N;
  F.G = G;
  F.means = host_f4(cfg->means);
  F.stds = host_f4(cfg->stds);
  TDN_LAUNCH(dd_target_fill_kernel, dim3(tdn_grid_1d(N, FILL_THREADS, FILL_MAX_BLOCKS), B), dim3(FILL_THREADS), 0,
             (hipStream_t)stream, F, (const int32_t*)assigned, labels, label_weights, bbox_targets, bbox_weights,
             (u64*)extra, num_pos, num_neg);
  TDN_LAUNCH_CHECK();
  return 0;
}
