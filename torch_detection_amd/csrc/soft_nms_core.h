// Soft-NMS of one sorted (image, class) segment: the device body of det_soft_nms_kernel (detect.hip).
// Scores change while it runs and the order of selection depends on the changed scores, so there is no mask + scan
// pair: one workgroup keeps the segment's boxes, areas and scores in registers and repeats
//   select  the alive candidate with the largest (order_key(score) << 32 | ~row): one arg-max over the workgroup;
//   decay   every other alive candidate that overlaps the winner has its score multiplied by the method's weight and
//           is dropped for good once the product is below min_score.
// The loop counter bounds the loop: every round retires one candidate, so a segment of n ends after at most n rounds
// whatever the boxes hold (NaN included).  Strict fp32 in the spec's operation order; the translation unit is compiled
// with -ffp-contract=off, and tests/soft_nms_ref.py repeats every operation in numpy float32, soft_exp included.
#pragma once
#include "nms_core.h"
#include "select_core.h"

constexpr int SOFT_PER = 4;                         // candidates per thread: 1024 * 4 = TDN_NMS_SEG_MAX
constexpr int SOFT_WAVE_MAX = 64 * SOFT_PER;        // the cut: a segment of at most this many runs in wave 0 alone
constexpr int SOFT_WAVES = BLK / 64;
static_assert(BLK * SOFT_PER == TDN_NMS_SEG_MAX, "one register slot per candidate of the longest segment");

struct SoftArgs {
  int32_t method;                                   // TDN_SOFT_NAIVE / LINEAR / GAUSSIAN
  float iou_thr, sigma, min_score;
};

// ---- soft_exp: e^x on [-64, 0] in fp32, operation for operation (relative error <= 4 * 2^-24) ----------
//   x <- min(max(x, -64), 0)                       (a NaN becomes -64)
//   k  = rint(x * LOG2E)                           round to nearest even, k in -93..0
//   r  = (x - k * LN2_HI) - k * LN2_LO             Cody-Waite: k * LN2_HI and the first difference are exact
//   p  = 1 + r (1 + r (C2 + r (C3 + r (C4 + r (C5 + r (C6 + r C7))))))    degree-7 Taylor, one product and one sum a step
//   e^x = p * 2^k                                  k added to the exponent field: p in [0.70, 1.42], the result is normal
constexpr float SOFT_LOG2E = 0x1.715476p+0f;
constexpr float SOFT_LN2_HI = 0x1.62e4p-1f;         // 15 significant bits
constexpr float SOFT_LN2_LO = 0x1.7f7d1cp-20f;
constexpr float SOFT_C2 = 0x1p-1f, SOFT_C3 = 0x1.555556p-3f, SOFT_C4 = 0x1.555556p-5f, SOFT_C5 = 0x1.111112p-7f,
                SOFT_C6 = 0x1.6c16c2p-10f, SOFT_C7 = 0x1.a01a02p-13f;

__device__ __forceinline__ float soft_exp(float x) {
  x = fminf(fmaxf(x, -64.0f), 0.0f);
  const float k = rintf(__fmul_rn(x, SOFT_LOG2E));
  const float t = __fsub_rn(x, __fmul_rn(k, SOFT_LN2_HI));
  const float r = __fsub_rn(t, __fmul_rn(k, SOFT_LN2_LO));
  float p = SOFT_C7;
  p = __fadd_rn(__fmul_rn(p, r), SOFT_C6);
  p = __fadd_rn(__fmul_rn(p, r), SOFT_C5);
  p = __fadd_rn(__fmul_rn(p, r), SOFT_C4);
  p = __fadd_rn(__fmul_rn(p, r), SOFT_C3);
  p = __fadd_rn(__fmul_rn(p, r), SOFT_C2);
  p = __fadd_rn(__fmul_rn(p, r), 1.0f);
  p = __fadd_rn(__fmul_rn(p, r), 1.0f);
  return __int_as_float(__float_as_int(p) + (int)k * (1 << 23));
}

// candidate b against the selected box a: w, h, inter, uni and ov are box_iou2(a, b)'s, operation for operation.  A pair
// that does not overlap (w == 0 or h == 0, NaN coordinates included) is left alone: false, *score untouched (and, as in
// soft_nms_cpu, not compared with min_score either); otherwise *score is multiplied by the method's weight
__device__ __forceinline__ bool soft_decay(const SoftArgs& P, const f32x4_t a, const float area_a, const f32x4_t b,
                                           const float area_b, float* score) {
  const float ltx = fmaxf(a[0], b[0]), lty = fmaxf(a[1], b[1]);
  const float rbx = fminf(a[2], b[2]), rby = fminf(a[3], b[3]);
  const float w = fmaxf(__fadd_rn(__fsub_rn(rbx, ltx), 1.0f), 0.0f);
  const float h = fmaxf(__fadd_rn(__fsub_rn(rby, lty), 1.0f), 0.0f);
  if (!(w > 0.0f && h > 0.0f)) return false;
  const float inter = __fmul_rn(w, h);
  const float uni = __fsub_rn(__fadd_rn(area_a, area_b), inter);
  const float ov = __fdiv_rn(inter, uni);
  float weight;
  if (P.method == TDN_SOFT_LINEAR) weight = ov > P.iou_thr ? __fsub_rn(1.0f, ov) : 1.0f;
  else if (P.method == TDN_SOFT_GAUSSIAN) weight = soft_exp(-__fdiv_rn(__fmul_rn(ov, ov), P.sigma));
  else weight = ov > P.iou_thr ? 0.0f : 1.0f;
  *score = __fmul_rn(weight, *score);
  return true;
}

struct SoftLds {                                    // the waves' winners of a round, double-buffered: one barrier a round
  u64 key[2][SOFT_WAVES];
  f32x4_t box[2][SOFT_WAVES];
};

__device__ __forceinline__ float soft_readlane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One segment of n >= 1 sorted candidates: sbox / srow / skey / sscore / kept point at the segment's first row, scol at
// the class's column of the dense scores (pitch C).  Candidate p sits in thread p % T, slot p / T.  WAVE: T = 64, wave 0
// alone (n <= SOFT_WAVE_MAX), no barrier; otherwise T = BLK, all 16 waves, one barrier a round.
// Writes kept[0, cnt) = the survivors' segment rows in selection order, kept[cnt, n) = -1, *num_kept = cnt, and for
// every row its final score and that score's order_key (a dropped row's are never read).
template <bool WAVE>
__device__ __forceinline__ void soft_nms_segment(const SoftArgs& P, const f32x4_t* __restrict__ sbox,
                                                 const int* __restrict__ srow, const float* __restrict__ scol, int C,
                                                 int n, uint32_t* __restrict__ skey, float* __restrict__ sscore,
                                                 int64_t* __restrict__ kept, int* __restrict__ num_kept, SoftLds* sh) {
  constexpr int T = WAVE ? 64 : BLK;
  const int t = threadIdx.x, wave = t >> 6;
  f32x4_t box[SOFT_PER];
  float area[SOFT_PER], sc[SOFT_PER];
  uint32_t row[SOFT_PER];
  unsigned alive = 0u;                              // bit e: slot e holds a candidate that is neither selected nor dropped
#pragma unroll
  for (int e = 0; e < SOFT_PER; ++e) {
    const int p = t + e * T;
    box[e] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    sc[e] = 0.f;
    row[e] = 0u;
    if (p < n) {
      box[e] = sbox[p];
      row[e] = (uint32_t)srow[p];
      sc[e] = scol[(size_t)row[e] * C];
      alive |= 1u << e;
    }
    area[e] = box_area(box[e]);
  }
  int cnt = 0;
  for (int it = 0; it < n; ++it) {                  // the counter bounds the loop: a round retires one candidate
    // ---- select ----
    u64 best = 0ull;                                // a real key is never 0: its low word is ~row, row < 2^31
    int be = 0;
#pragma unroll
    for (int e = 0; e < SOFT_PER; ++e) {
      const u64 k = (alive >> e & 1u) ? compose(order_key(sc[e]), row[e]) : 0ull;
      if (k > best) {
        best = k;
        be = e;
      }
    }
    u64 win = best;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const u64 other = __shfl_xor(win, o, 64);
      win = other > win ? other : win;
    }
    f32x4_t sel = {0.f, 0.f, 0.f, 0.f};
    if (win != 0ull) {                              // wave-uniform; keys are distinct: one lane owns the winner
      f32x4_t mine = box[0];
#pragma unroll
      for (int e = 1; e < SOFT_PER; ++e)
        if (be == e) mine = box[e];
      const int owner = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(best == win)) - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) sel[j] = soft_readlane(mine[j], owner);
    }
    if constexpr (!WAVE) {
      const int buf = it & 1;
      if ((t & 63) == 0) {
        sh->key[buf][wave] = win;
        sh->box[buf][wave] = sel;
      }
      __syncthreads();
      // buffer `buf` is written again in round it + 2, which a wave reaches only through the barrier of round it + 1:
      // every wave has read this round's winners by then
      win = 0ull;
      int ww = 0;
#pragma unroll
      for (int i = 0; i < SOFT_WAVES; ++i) {
        const u64 k = sh->key[buf][i];
        if (k > win) {
          win = k;
          ww = i;
        }
      }
      sel = sh->box[buf][ww];
    }
    if (win == 0ull) break;                         // nobody is alive: the same for every thread
    if (best == win) {                              // the one thread that holds the winner retires it
      alive &= ~(1u << be);
      kept[cnt] = (int64_t)(t + be * T);
    }
    ++cnt;
    // ---- decay ----
    const float area_s = box_area(sel);
#pragma unroll
    for (int e = 0; e < SOFT_PER; ++e)
      if (alive >> e & 1u) {
        float v = sc[e];
        if (soft_decay(P, sel, area_s, box[e], area[e], &v)) {
          sc[e] = v;
          if (v < P.min_score) alive &= ~(1u << e);
        }
      }
  }
#pragma unroll
  for (int e = 0; e < SOFT_PER; ++e) {
    const int p = t + e * T;
    if (p < n) {
      skey[p] = order_key(sc[e]);
      sscore[p] = sc[e];
    }
  }
  for (int k = cnt + t; k < n; k += T) kept[k] = -1;
  if (t == 0) *num_kept = cnt;
}
