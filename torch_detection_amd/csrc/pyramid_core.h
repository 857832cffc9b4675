// The pyramid-wide kernels, stated once: dense_head.hip (§4k), pyramid_conv.hip (§4m), pyramid_gn.hip (§4o)
// and bfp.hip (§4r) number their workgroups over the concatenated pieces of up to 8 levels and look the level up in a
// `first` table that travels in the kernel arguments.  The two GEMM files also share the pieces of the transposing
// weight-gradient product over plain-store LDS tiles and the host side of the cut: slice length, `first` tables, workspace
// layout, plan words 12..15.  Each file supplies its argument struct, its forward / dgrad kernels, what a step loads and
// stores (load_tile / store_tile), its lane offsets, where a lane's result goes, and its own limits.
#pragma once
#include "common.h"

// ---- device -------------------------------------------------------------------------------------------------------------
// the level that workgroup / slice b belongs to: the last one whose first index is <= b, a scan of at most 8 entries; an
// empty level shares its `first` with the next one and owns no index
__device__ __forceinline__ int find_level(const int* first, int n, int b) {
  int l = 0;
  for (int i = 1; i < n; ++i)
    if (b >= first[i]) l = i;
  return __builtin_amdgcn_readfirstlane(l);
}

__device__ __forceinline__ bf16x8_t zero8() { return __builtin_bit_cast(bf16x8_t, (s16x8_t){0, 0, 0, 0, 0, 0, 0, 0}); }

// ---- the transposing weight-gradient product: D[c][o] += sum_m x[m][c] * g[m][o] ----------------------------------------
// 256 threads, steps of LEVEL_TILE rows.  Two LDS tiles written with plain stores: x [128][64 channels] with XRB row bytes
// and g [128][16 NB columns] with GRB row bytes (the data bytes + a 32-byte pad, which spreads 4 rows over distinct
// banks), read back transposed (ds_read_b64_tr_b16).  Wave w owns channels 16 w .. + 15 and all 16 NB columns.
//
// The kernel keeps its accumulators, indexes them itself and computes its own lane offsets: a callee that loops over an
// accumulator array is unrolled before it is inlined, the array then becomes one 16-float vector and the kernel 72 VGPRs
// larger (profiles/pyramid_core_refactor_checks.md).  So the slice loop below takes the kernel's `mma(i, xf, gp)` as it
// takes its load_tile / store_tile, and the kernel writes that lambda as one call of wg_mma on its acc[i], acc1[i].
constexpr int LEVEL_TILE = 128;            // rows per workgroup (forward, dgrad), rows per weight-gradient step

// one transposed fragment (ds_read_b64_tr_b16): rows r .. r + 3 and r + 4 .. r + 7 of a tile with RB row bytes, p at row r
template <int RB>
__device__ __forceinline__ bf16x8_t wg_frag(const char* p) {
  const s16x4_t lo = lds_read_tr16(p);
  const s16x4_t hi = lds_read_tr16(p + 4 * RB);
  return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// the x operand of the column sums
template <bool F16>
__device__ __forceinline__ bf16x8_t wg_ones() {
  bf16x8_t ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = f32_to_elem<F16>(1.0f);
  return ones;
}

// one 16-column block of g at gp against the x fragment: D[row = channel][col = o]; with do_colsum also its column sums
template <bool F16, int GRB>
__device__ __forceinline__ void wg_mma(const bf16x8_t& xf, const char* gp, bool do_colsum, const bf16x8_t& ones,
                                       f32x4_t& acc, f32x4_t& acc1) {
  const bf16x8_t gf = wg_frag<GRB>(gp);
  acc = mfma16<F16>(xf, gf, acc);
  if (do_colsum) acc1 = mfma16<F16>(ones, gf, acc1);
}

// T steps from row m_begin of the slice.  load_tile(first row) fetches a step into the kernel's registers (zeros past the
// slice), store_tile() writes them to the two tiles; the next step's loads are in flight under the MFMAs.
template <int NB, int XRB, int GRB, class Load, class Store, class Mma>
__device__ __forceinline__ void wg_slice(const char* sH, const char* sG, int64_t m_begin, int T, Load load_tile,
                                         Store store_tile, int x_off, int g_off, Mma mma) {
  if (T > 0) {
    load_tile(m_begin);
    store_tile();
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const bool more = t + 1 < T;
      if (more) load_tile(m_begin + (int64_t)(t + 1) * LEVEL_TILE);
#pragma unroll
      for (int kk = 0; kk < LEVEL_TILE / 32; ++kk) {
        const bf16x8_t xf = wg_frag<XRB>(sH + x_off + kk * 32 * XRB);
#pragma unroll
        for (int i = 0; i < NB; ++i) mma(i, xf, sG + g_off + i * 32 + kk * 32 * GRB);
      }
      __syncthreads();                      // every wave has read step t
      if (more) store_tile();
      __syncthreads();
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int check_levels(const char* who, int n, int max_levels) {
  TDN_CHECK(n >= 1 && n <= max_levels, "%s: num_levels=%d out of 1..%d", who, n, max_levels);
  return 0;
}
// `what`: "row" or "pixel"
inline int check_tiles(const char* who, int64_t tiles, const char* what) {
  TDN_CHECK(tiles < ((int64_t)1 << 28), "%s: %lld %s tiles in all, at most 2^28 - 1", who, (long long)tiles, what);
  return 0;
}

// the slice length depends on the shapes alone: about `target` slices of the total, whole steps, at least one
inline int64_t slice_len(int64_t total, int target, int step) {
  int64_t sr = (total + target - 1) / target;
  sr = (sr + step - 1) / step * step;
  return sr < step ? step : sr;
}

// first[l] = the `unit`-row pieces of the levels before l, for l in 0 .. max_levels (past n: all of them); -> their number.
// first may be NULL.
inline int64_t fill_first(const int64_t* rows, int n, int64_t unit, int* first, int max_levels) {
  int64_t count = 0;
  for (int l = 0; l <= max_levels; ++l) {
    if (first) first[l] = (int)count;
    if (l < n) count += (rows[l] + unit - 1) / unit;
  }
  return count;
}

// The cut of a product over the levels: LEVEL_TILE-row tiles (forward, dgrad) or slices of about 1 / target of the rows
// (wgrad, two launches: slabs, then the finalize, which also runs alone over an empty pyramid); `first` is the table of
// the kind at hand.
struct LevelCut { int tiles, slices, slice_rows, launches; };
inline LevelCut cut_levels(bool wgrad, const int64_t* rows, int n, int target, int* first, int max_levels) {
  int64_t total = 0;
  for (int l = 0; l < n; ++l) total += rows[l];
  LevelCut c;
  c.slice_rows = (int)slice_len(total, target, LEVEL_TILE);
  c.tiles = (int)fill_first(rows, n, LEVEL_TILE, wgrad ? nullptr : first, max_levels);
  c.slices = (int)fill_first(rows, n, c.slice_rows, wgrad ? first : nullptr, max_levels);
  c.launches = wgrad ? (c.slices > 0 ? 2 : 1) : (c.tiles > 0 ? 1 : 0);
  return c;
}

// workspace of a weight gradient: slab [slice][cols][...] | colsum [slice][cols]; nothing for `slices` == 0
struct SlabWs { float* slab; float* colsum; int64_t bytes; };
inline SlabWs slab_layout(int slices, int64_t slab_bytes, int cols, void* base) {
  tdn_carver c{(char*)base, 0};
  SlabWs w{nullptr, nullptr, 0};
  if (slices > 0) {
    w.slab = c.take<float>(slab_bytes / 4);
    w.colsum = c.take<float>((int64_t)slices * cols);
  }
  w.bytes = c.off;
  return w;
}

// a 64-bit size in a plan record: its low 31 bits, then the rest (_lib.size_word reads it); words 12..15 of the 16-word
// records are the slab and workspace bytes
inline void put_size(int32_t* out, int64_t v) {
  out[0] = (int32_t)(v & 0x7fffffff);
  out[1] = (int32_t)(v >> 31);
}
inline void put_sizes(int32_t* out, int64_t slab_bytes, int64_t ws) {
  put_size(out + 12, slab_bytes);
  put_size(out + 14, ws);
}
