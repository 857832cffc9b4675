// The 128 x 128 x 64 ring GEMMs of the heads, stated once: linear.hip (§4i) and deconv.hip (§4j) take the tile constants,
// the two-slot LDS ring with its counted wait, the swizzles, both MFMA loops and the host-side split rule, plan record
// and weight-gradient launch from here, and supply their stage_load (where a row's source pointer comes from), their
// slicing and their epilogues.  DESIGN.md §4i "The shared core": why the lane arithmetic is scalar functions.
#pragma once
#include "common.h"

constexpr int NT = 256;                    // threads per workgroup: 4 waves as 2 x 2
constexpr int BM = 128, BN = 128, BK = 64; // output tile and reduction step of every product
constexpr int TILE_BYTES = BM * BK * 2;    // one operand, one step: 16 KB
constexpr int STAGE = 2 * TILE_BYTES;
constexpr int NST = 2;                     // ring slots: the loads of NST - 1 steps are in flight while one is multiplied.
                                           // Measured: a CU cannot pull the 32 KB a 128 x 128 x 64 step needs
                                           // faster than it multiplies it, so 4 slots (one workgroup per CU) were slower on
                                           // every many-tile product than 2 slots (two workgroups per CU)
constexpr int LOADS = 8;                   // LDS-DMA instructions per wave and step (4 per operand)
constexpr int LDS_BYTES = NST * STAGE;     // 64 KB: two workgroups per CU
constexpr int FILL_WGS = 256;              // the split rule aims at one workgroup per CU

// Every wave issues exactly LOADS LDS-DMA instructions per step (rows or steps past the end read the zero page), so a
// counted wait retires a step: with the NST - 2 youngest steps left in flight, the oldest one has landed; the barrier
// then makes every wave's share of it visible and frees the slot that was multiplied last.
__device__ __forceinline__ void wait_step_and_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LOADS * (NST - 2)) : "memory");
}

// ---- the K-contiguous product: C[m][n] = sum_k A[m][k] * B[n][k] --------------------------------------------------------
// Loader: one wave-instruction fills 8 rows x 128 bytes; LDS position c of row r holds source piece c ^ (r & 7).  Lane
// l of wave w, lrow = l >> 3: 8 elements from column kc_src_el of row kc_row, LDS base kc_dst bytes into the tile.
__device__ __forceinline__ int kc_row(int it, int wave, int lrow) { return (it * 4 + wave) * 8 + lrow; }
__device__ __forceinline__ int kc_src_el(int lane, int lrow) { return ((lane & 7) ^ lrow) * 8; }
__device__ __forceinline__ int kc_dst(int it, int wave) { return (it * 4 + wave) * 1024; }

// Fragment reads: lane l takes row fr = l & 15, k pieces fq = l >> 4 and 4 + fq of the step; wave (wm, wn) = (w >> 1, w & 1)
// takes rows wm * 64 .. + 63 of A and wn * 64 .. + 63 of B.  Byte offsets into a ring slot.
__device__ __forceinline__ int kc_a_off(int wm, int i, int fr) { return (wm * 64 + i * 16 + fr) * 128; }
__device__ __forceinline__ int kc_b_off(int wn, int j, int fr) { return TILE_BYTES + (wn * 64 + j * 16 + fr) * 128; }
__device__ __forceinline__ int kc_k_off(int kk, int fq, int fr) { return ((kk * 4 + fq) ^ (fr & 7)) * 16; }

// Runs chunks c_begin .. c_end - 1 (at least one) through the ring.  stage_load(chunk, slot) issues the LOADS LDS-DMA
// instructions of one step, also for a chunk >= c_end (from the zero page: the vmcnt bookkeeping stays uniform).
// acc[i][j] is D[row = n][col = m]: a lane gets 4 consecutive n, wn * 64 + j * 16 + fq * 4 .., of m = wm * 64 + i * 16 + fr.
template <bool F16, class Load>
__device__ __forceinline__ void kc_ring(const char* smem, int c_begin, int c_end, Load stage_load, const int (&a_off)[4],
                                        const int (&b_off)[4], const int (&k_off)[2], f32x4_t (&acc)[4][4]) {
#pragma unroll
  for (int s = 0; s < NST - 1; ++s) stage_load(c_begin + s, s);
  int slot = 0, fill = NST - 1;
  for (int c = c_begin; c < c_end; ++c) {
    wait_step_and_barrier();                        // step c has landed for every wave; the slot of step c - 1 is free
    stage_load(c + NST - 1, fill);
    const char* st = smem + slot * STAGE;
    slot = (slot + 1 == NST) ? 0 : slot + 1;
    fill = (fill + 1 == NST) ? 0 : fill + 1;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8_t af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds_read_b128(st + a_off[i] + k_off[kk]);
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = lds_read_b128(st + b_off[j] + k_off[kk]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16<F16>(bf[j], af[i], acc[i][j]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dummy tail loads still target the ring
}

// ---- the transposed (weight-gradient) product: D[o][k] = sum_m g[m][o] * x[m][k] ----------------------------------------
constexpr int TR_RB = 256;                 // row bytes of both tiles: 128 columns

// 32-byte-chunk XOR swizzle of a 256-byte row read with ds_read_b64_tr_b16
__device__ __forceinline__ int tr_swz(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

// Loader: one wave-instruction fills 4 rows x 256 bytes.  Lane l of wave w, lrow = l >> 4, pc = l & 15: 8 elements from
// column tr_src_el of row it * 16 + tr_row0 of a 64-row step, LDS base tr_dst bytes into the tile.
__device__ __forceinline__ int tr_row0(int wave, int lrow) { return wave * 4 + lrow; }
__device__ __forceinline__ int tr_src_el(int pc, int row0) { return ((((pc >> 1) ^ tr_swz(row0)) << 1) | (pc & 1)) * 8; }
__device__ __forceinline__ int tr_dst(int it, int wave) { return (it * 16 + wave * 4) * TR_RB; }

// Fragment reads (ds_read_b64_tr_b16): lane group q4 = l >> 4 takes rows rrow = 8 * q4 + ((l & 15) >> 2) (+ kk * 32 + 4 *
// half) of a 32-row half step, 4 columns from pp = l & 3 of the 16-column group `col16`; f = tr_swz(rrow).
__device__ __forceinline__ int tr_off(int rrow, int col16, int f, int pp) { return rrow * TR_RB + ((col16 ^ f) << 5) + pp * 8; }

// One 64-row step from ring slot st.  g_off / x_off: tr_off of the wave's 16-column groups wm * 4 + i of g and wn * 4 + j
// of x (+ TILE_BYTES).  acc[i][j] is D[row = column of x][col = column of g]: x columns wn * 64 + j * 16 + q4 * 4 .. + 3 of
// g column wm * 64 + i * 16 + (l & 15); with do_colsum, acc1[i][0] of lanes with q4 == 0 is that g column's sum (x ones).
template <bool F16>
__device__ __forceinline__ void tr_step(const char* st, const int (&g_off)[4], const int (&x_off)[4], bool do_colsum,
                                        const bf16x8_t& ones, f32x4_t (&acc)[4][4], f32x4_t (&acc1)[4]) {
  constexpr int RB = TR_RB;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    bf16x8_t gf[4], xf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const s16x4_t lo = lds_read_tr16(st + g_off[i] + kk * 32 * RB);
      const s16x4_t hi = lds_read_tr16(st + g_off[i] + (kk * 32 + 4) * RB);
      gf[i] = __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const s16x4_t lo = lds_read_tr16(st + x_off[j] + kk * 32 * RB);
      const s16x4_t hi = lds_read_tr16(st + x_off[j] + (kk * 32 + 4) * RB);
      xf[j] = __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma16<F16>(xf[j], gf[i], acc[i][j]);
    if (do_colsum) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc1[i] = mfma16<F16>(ones, gf[i], acc1[i]);
    }
  }
}

// Runs T >= 1 steps of BK rows from row m_begin through the ring.  stage_load(first row, slot) issues the LOADS LDS-DMA
// instructions of a step, rows past the slice from the zero page.  (T computed in here changes linear_wgrad's registers.)
template <bool F16, class Load>
__device__ __forceinline__ void tr_ring(const char* smem, int m_begin, int T, Load stage_load, const int (&g_off)[4],
                                        const int (&x_off)[4], bool do_colsum, const bf16x8_t& ones,
                                        f32x4_t (&acc)[4][4], f32x4_t (&acc1)[4]) {
#pragma unroll
  for (int s = 0; s < NST - 1; ++s) stage_load(m_begin + s * BK, s);
  int slot = 0, fill = NST - 1;
  for (int t = 0; t < T; ++t) {
    wait_step_and_barrier();
    stage_load(m_begin + (t + NST - 1) * BK, fill);
    const char* st = smem + slot * STAGE;
    slot = (slot + 1 == NST) ? 0 : slot + 1;
    fill = (fill + 1 == NST) ? 0 : fill + 1;
    tr_step<F16>(st, g_off, x_off, do_colsum, ones, acc, acc1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dummy tail loads still target the ring
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static inline int round64(int v) { return (v + 63) & ~63; }
static inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The split rule: a reduction of `chunks` steps of BK is cut into slices of whole chunks.  `forced` > 0 asks for that many.
// Otherwise `tiles` >= `fill` is not cut, fewer aim at FILL_WGS workgroups with >= `min_cps` chunks per slice.  Empty: 0.
struct Split { int cps, slices; };
static inline Split split_rule(int tiles, int chunks, int forced, int fill, int min_cps) {
  int want = 1;
  if (forced > 0) want = forced;
  else if (tiles > 0 && tiles < fill) {
    want = FILL_WGS / tiles;
    if (want > chunks / min_cps) want = chunks / min_cps;
  }
  if (want > chunks) want = chunks;
  if (want < 1) want = 1;
  Split s;
  s.cps = chunks > 0 ? (chunks + want - 1) / want : 0;
  s.slices = chunks > 0 ? (chunks + s.cps - 1) / s.cps : 0;
  return s;
}

// The 16-word record of tdn_linear_plan / tdn_deconv2x2_plan; a 64-bit size is split into its low 31 bits and the rest.
static inline void write_plan(int32_t* out, int tiles_r, int tiles_c, int slices, int cps, int chunks, int workgroups,
                              int launches, int flags, int64_t slab_bytes, int64_t ws) {
  out[0] = BM; out[1] = BN; out[2] = BK;
  out[3] = tiles_r; out[4] = tiles_c; out[5] = tiles_r * tiles_c;
  out[6] = slices; out[7] = cps; out[8] = chunks;
  out[9] = workgroups;
  out[10] = launches;
  out[11] = flags;
  out[12] = (int32_t)(slab_bytes & 0x7fffffff); out[13] = (int32_t)(slab_bytes >> 31);
  out[14] = (int32_t)(ws & 0x7fffffff); out[15] = (int32_t)(ws >> 31);
}

// A weight gradient: `wgs` workgroups of the dtype's kernel (none when 0), then FINALIZE over fin_elems (none when 0).
template <auto KERNEL_F16, auto KERNEL_BF16, auto FINALIZE, class Args>
int launch_wgrad(const char* what, bool f16, int wgs, const Args& p, int64_t fin_elems, int slices, hipStream_t stream) {
  if (wgs > 0) {
    if ((f16 ? tdn_allow_lds<KERNEL_F16>(LDS_BYTES, what) : tdn_allow_lds<KERNEL_BF16>(LDS_BYTES, what)) < 0) return -1;
    const dim3 grid((unsigned)wgs);
    if (f16) TDN_LAUNCH(KERNEL_F16, grid, dim3(NT), LDS_BYTES, stream, p);
    else TDN_LAUNCH(KERNEL_BF16, grid, dim3(NT), LDS_BYTES, stream, p);
    TDN_LAUNCH_CHECK();
  }
  if (fin_elems > 0) {
    const int fgrid = tdn_grid_1d(fin_elems, NT, 4096);
    TDN_LAUNCH(FINALIZE, dim3(fgrid), dim3(NT), 0, stream, p, slices);
    TDN_LAUNCH_CHECK();
  }
  return 0;
}
