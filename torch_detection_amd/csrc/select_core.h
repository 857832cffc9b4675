// Workgroup-wide selection pieces shared by the RPN proposal pipeline (proposal.hip), the training-target sampler
// (target.hip) and the test-time detections (detect.hip): the order-preserving score keys, the exclusive scan in thread
// order, the radix select of the k-th highest 32-bit key, the LDS bitonic sort and the top-k built from them.  Integer
// LDS atomics only count, so every result is a pure function of the keys.
#pragma once
#include "common.h"

typedef unsigned long long u64;

// ---- keys ----------------------------------------------------------------------------------------------------
// order-preserving: a > b (as floats, -0 == +0)  <=>  order_key(a) > order_key(b)
__device__ __forceinline__ uint32_t order_key(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ u64 compose(uint32_t key, uint32_t i) { return ((u64)key << 32) | (uint32_t)~i; }

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

// ---- sort and top-k (1024 threads) ---------------------------------------------------------------------------------
// descending bitonic sort of s[0, P), P a power of two
__device__ __forceinline__ void block_sort_desc(u64* s, int P) {
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += BLK) {
        const int i = 2 * t - (t & (stride - 1));
        const int j = i + stride;
        const u64 a = s[i], c = s[j];
        if ((a < c) == ((i & size) == 0)) {
          s[i] = c;
          s[j] = a;
        }
      }
      __syncthreads();
    }
}

__host__ __device__ __forceinline__ int pow2_ceil(int m) {
  int p = 1;
  while (p < m) p <<= 1;
  return p;
}

// The k highest of n keys (ties: lower index first) as composite keys (key << 32 | ~index), sorted descending into
// skeys[0, pow2_ceil(k)) (zero padding).  F(i0, cnt, keys) fetches keys i0 .. i0+cnt-1 (cnt <= TK_PER).  Returns
// min(n, k).  hist: TK_BINS ints of LDS, misc: TK_MISC ints.
template <class Fetch>
__device__ int block_topk(const Fetch& F, int n, int k, u64* skeys, int* hist, int* misc) {
  const int tid = threadIdx.x;
  int m;
  if (n <= k) {
    for (int i0 = tid * TK_PER; i0 < n; i0 += TK_STEP) {
      const int cnt = min(TK_PER, n - i0);
      uint32_t kk[TK_PER];
      F(i0, cnt, kk);
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) skeys[i0 + e] = compose(kk[e], i0 + e);
    }
    m = n;
  } else {
    // radix select of the threshold key T: k - need keys are > T, and the first `need` keys == T are taken
    int need;
    const uint32_t T = block_radix_threshold(F, n, k, hist, misc, &need);
    // ordered compaction: keys > T go to [0, k - need) in any order (the sort below orders them), the first `need`
    // keys == T in index order to [k - need, k)
    const int ngt = k - need;
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
      int tot;   // both counts packed: a step holds at most 8192 of either
      const int ex = block_excl_scan(ng | (nt << 16), misc, &tot);
      int gpos = gt_done + (ex & 0xFFFF), tpos = ties_done + (ex >> 16);
#pragma unroll
      for (int e = 0; e < TK_PER; ++e)
        if (e < cnt) {
          if (kk[e] > T) {
            skeys[gpos++] = compose(kk[e], i0 + e);
          } else if (kk[e] == T) {
            if (tpos < need) skeys[ngt + tpos] = compose(kk[e], i0 + e);
            ++tpos;
          }
        }
      gt_done += tot & 0xFFFF;
      ties_done += tot >> 16;
    }
    m = k;
  }
  const int P = pow2_ceil(m);
  for (int i = m + tid; i < P; i += BLK) skeys[i] = 0ull;   // below every real key
  block_sort_desc(skeys, P);
  return m;
}
