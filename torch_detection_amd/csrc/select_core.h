// Workgroup-wide selection pieces shared by the RPN proposal pipeline (proposal.hip) and the training-target sampler
// (target.hip): the exclusive scan in thread order and the radix select of the k-th highest 32-bit key.  Integer LDS
// atomics only count, so every result is a pure function of the keys.
#pragma once
#include "common.h"

constexpr int BLK = 1024;
constexpr int TK_PER = 8;                     // keys per thread per step, consecutive: one scan orders a whole step
constexpr int TK_STEP = BLK * TK_PER;
constexpr int TK_BINS = 2048;                 // 11-bit digits: 21..31, 10..20, 0..9
constexpr int TK_MISC = 64;                   // ints of scratch: [0,16) scan, [16,18) bin choice, [32,64) caller

// exclusive prefix sum over the workgroup in thread order; *total = the sum of all
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < BLK / 64; ++w) {
    const int c = sh[w];
    before += (w < wave) ? c : 0;
    tot += c;
  }
  __syncthreads();
  *total = tot;
  return before + incl - v;
}

// Radix select of the threshold key T among n > k >= 1 keys: k - *need keys are > T, and the first *need keys == T (in
// index order) complete the k highest.  F(i0, cnt, keys) fetches keys i0 .. i0+cnt-1 (cnt <= TK_PER).  hist: TK_BINS
// ints of LDS, misc: TK_MISC ints.  Every thread of the 1024 returns the same T and *need.
template <class Fetch>
__device__ __forceinline__ uint32_t block_radix_threshold(const Fetch& F, int n, int k, int* hist, int* misc,
                                                          int* need_out) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0u, pmask = 0u;
  int need = k;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const uint32_t dmask = pass == 2 ? 0x3FFu : 0x7FFu;
    for (int b = tid; b < TK_BINS; b += BLK) hist[b] = 0;
    __syncthreads();
    for (int i0 = tid * TK_PER; i0 < n; i0 += TK_STEP) {
      const int cnt = min(TK_PER, n - i0);
      uint32_t kk[TK_PER];
      F(i0, cnt, kk);
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt && (kk[e] & pmask) == prefix) atomicAdd(&hist[(kk[e] >> shift) & dmask], 1);
    }
    __syncthreads();
    // thread t owns bins 2047-2t and 2046-2t: an exclusive scan in thread order counts the keys in higher bins
    const int hi = TK_BINS - 1 - 2 * tid;
    const int ch = hist[hi], cl = hist[hi - 1];
    int tot;
    const int above = block_excl_scan(ch + cl, misc, &tot);
    if (above < need && need <= above + ch) {
      misc[16] = hi;
      misc[17] = above;
    } else if (above + ch < need && need <= above + ch + cl) {
      misc[16] = hi - 1;
      misc[17] = above + ch;
    }
    __syncthreads();
    need -= misc[17];
    prefix |= (uint32_t)misc[16] << shift;
    pmask |= dmask << shift;
    __syncthreads();
  }
  *need_out = need;
  return prefix;
}
