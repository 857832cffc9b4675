// Implicit-GEMM convolution on MFMA (gfx950): forward and input-gradient of the ResNet/FPN convs.
//
// Replaces nn.Conv2d.forward (+ folded eval BatchNorm2d, residual add, ReLU) as called from
// models/backbone/resnet.py:42-59,97-119,253-258 and models/necks/fpn.py:92-108, and its autograd
// input gradient.  GEMM view:  D[n][m] = sum_k W[n][k] * X[m][k]
//   m = output pixel (N*Ho*Wo),  n = output channel,  k = (tap, input channel)
// X rows are gathered on the fly from the NHWC activation (one contiguous BK-channel run per tap),
// W rows are the K-major packed weights.  Both tiles go global -> LDS with 16-byte LDS-DMA
// (global_load_lds_dwordx4), XOR-swizzled on the *source* address so that the ds_read_b128 fragment
// reads are bank-conflict free; the accumulator is kept as D[channel][pixel] so each lane owns 4
// consecutive channels of one pixel (8-byte NHWC stores, float4 scale/shift loads).
//
// A "class" is a sub-lattice of output pixels sharing one tap list: forward and stride-1 dgrad have one
// class; stride-2 dgrad has four output-parity classes (gather form, no atomics, no zero-insertion).
#include "conv_host.h"

// conv_halo.hip: LDS-resident activation patch kernel for 3x3 / 1x1 convs (stride-1 3x3, any 1x1 forward; stride-1
// input gradients).  Each returns 1 when it launched, 0 when the shape stays with the generic kernel below.
int tdn_halo_conv_fwd(const void* x, const void* w_fwd, void* y, int N, int H, int W, int Cin, int Cout, int k,
                      int stride, int pad, const tdn_epilogue* ep, int dtype, hipStream_t stream);
int tdn_halo_conv_dgrad(const void* g, const void* w_dgrad, void* dx, int N, int H, int W, int Cin, int Cout, int k,
                        int stride, int pad, const tdn_epilogue* ep, int dtype, hipStream_t stream);
int tdn_halo_plan(int kind, int N, int H, int W, int Cin, int Cout, int k, int stride, int pad, int32_t* o);

struct GemmClass {
  int Ha, Wa, M;     // rows m -> (img, a, b) over an Ha x Wa lattice; M = N*Ha*Wa
  int oh0, ow0;      // output pixel = (a*so + oh0, b*so + ow0)
  int ntaps;
  int taps[9];       // (dh+64) | (dw+64)<<8 | widx<<16 ; input pixel = (a*sa + dh, b*sa + dw)
  unsigned mul_hw, shr_hw, mul_w, shr_w;   // exact division of m < 2^31 by Ha*Wa and by Wa: umulhi + shift
};

// n / d with the (mul, shr) pair of fast_div_init (conv_host.h)
__device__ __forceinline__ int fast_div(int n, unsigned mul, unsigned shr) {
  return mul ? (int)(__umulhi((unsigned)n, mul) >> shr) : n;
}

struct GemmParams {
  const bf16_t* in;
  const bf16_t* wt;
  bf16_t* out;
  const float* scale;
  const float* shift;
  const bf16_t* addend;
  const bf16_t* mask;
  int Hin, Win, Cpix, Ktap, wt_row;
  int Hout, Wout, Cout;
  int sa, so;
  int addend_mode, addend_h, addend_w, relu, out_f32;
  int tiles_n, nwg_pad;
  unsigned tn_mul, tn_shr;   // fast_div by tiles_n
  int ncls;
  int grouped;   // block-diagonal grouped conv: the output tile's 64 channels see only the same 64 input channels
  GemmClass cls[4];
};

template <int BK>
__device__ __forceinline__ int swz_f(int row) {
  if constexpr (BK == 128) return row & 15;        // 256-byte rows: every row starts at bank 0, 16 chunks
  else if constexpr (BK == 64) return (row >> 1) & 7;
  else return (4 - ((row >> 2) & 3)) & 3;
}

// Counted wait on the vector-memory queue + workgroup barrier in ONE asm statement: the compiler may not move
// LDS reads / LDS-DMA issues across it, and it does not drain the DMA queue (a __syncthreads() would).
template <int N>
__device__ __forceinline__ void wait_vm_and_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// <BM x BN> output tile (pixels x channels), BK-deep K-steps, WM x WN waves (wave tile BM/WM x BN/WN),
// NSTAGE-deep LDS ring filled by LDS-DMA: while K-step t is multiplied, the loads of steps t+1 .. t+NSTAGE-2 stay
// in flight (counted vmcnt, one s_barrier per K-step).
// MODE 0: fragments read per 32-deep sub-step;  MODE 6: sub-step 1's fragment reads issued under sub-step 0's MFMAs.
// (Measured and dropped, DESIGN.md §6: mid-step DMA issue, reads-first, phase-staggered wave groups, BK = 32 rings.)
// (Register staging — global_load_dwordx4 -> VGPR -> ds_write_b128 — measured the same as LDS-DMA and was dropped;
// buffer_load ... lds with the hardware range check was 15-25 % slower.  DESIGN.md §6.)
// TAG only changes the kernel's symbol name: TAG 1 is the instantiation bench.py requests (TDN_TAG_DOMINANT) for the
// launches of the heaviest shape of the net (3x3, 256 -> 256 at M >= 100000: neck.fpn_convs.0 forward and its dgrad)
// that it brackets with HIP events, so that rocprofv3 --stats of the same command reports exactly those launches on a
// line of their own, directly comparable with bench.py's figure.
// KG > 1: in-workgroup split-K.  The workgroup holds KG groups of WM x WN waves; group g owns its own LDS ring and
// multiplies K-steps g, g+KG, g+2KG, ... of the SAME output tile; the KG partial accumulators are summed through LDS
// in a fixed order and the epilogue is shared out over the groups.  Reason (cycle stamps): one
// wave sustains only ~4 B/clk of LDS-DMA however many loads it keeps in flight, a CU needs ~16 loading waves to reach
// its ~40 B/clk L2->LDS rate, and the small-M layers (layer3/4, FPN top levels) have too few output tiles to put
// four 4-wave workgroups on every CU — so the extra waves are recruited along K instead.
template <int BM, int BN, int BK, int WM, int WN, int NSTAGE, int MODE = 0, int TAG = 0, int KG = 1, bool F16 = false>
__global__ __launch_bounds__(WM * WN * KG * 64) void conv_gemm_kernel(const GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem_all[];
  constexpr int NW = WM * WN;
  constexpr int ROWB = BK * 2;
  constexpr int CH = BK / 8;
  constexpr int RPI = 64 / CH;
  constexpr int A_IT = BM / (RPI * NW);
  constexpr int B_IT = BN / (RPI * NW);
  constexpr int LOADS = A_IT + B_IT;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
  constexpr int WTM = BM / WM, WTN = BN / WN, FM = WTM / 16, FN = WTN / 16;
  constexpr int KSUB = BK / 32;
  static_assert(A_IT >= 1 && B_IT >= 1 && FM >= 1 && FN >= 1, "tile too small for this wave layout");
  static_assert(BM % (RPI * NW) == 0 && BN % (RPI * NW) == 0, "loader does not tile evenly");
  static_assert(NSTAGE >= 2 && LOADS * (NSTAGE - 2) < 64, "vmcnt immediate out of range");
  static_assert(KG == 1 || BM * BN * 4 <= NSTAGE * STAGE, "partial sums must fit the group's LDS ring");
  constexpr bool EARLY_EPI = FN * FM <= 8;   // small tiles: fetch scale/shift before the K loop (registers to spare)
  // WIDE: the MFMA rows of channel-fragment i are weight rows  q*4FN + 4i + e  (q = row>>2, e = row&3) of the wave's
  // channel block instead of 16i + row, so a lane's FN fragments of one pixel are 4FN CONSECUTIVE channels: the
  // epilogue then moves 8FN contiguous bytes per lane (scale/shift, residual, ReLU mask, store) instead of FN
  // scattered 8-byte pieces — the store tail of a 192x256 tile was 11 % of the kernel (cycle stamps).
  // The weight tile gets its own XOR swizzle (swz_w) so that this row pattern still reads LDS conflict-free.
  constexpr bool WIDE = (BK >= 64) && (FN == 2 || FN == 4);
  constexpr int CPL = 4 * FN;                // channels per lane and pixel
  constexpr bool OWN_BY_J = (KG == 1) || (FM % KG == 0);   // split-K groups share the epilogue by pixel fragment

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = KG == 1 ? 0 : wave_all / NW;     // split-K group of this wave
  const int wave = KG == 1 ? wave_all : wave_all % NW;   // wave index inside its group
  char* smem = smem_all + grp * (NSTAGE * STAGE);
  const GemmClass& c = p.cls[blockIdx.y];
  int taps_s[9];   // the class's tap table in scalar registers: nine loads in flight at once, one wait
#pragma unroll
  for (int i = 0; i < 9; ++i) taps_s[i] = c.taps[i];
  const int ntaps = c.ntaps;
  const int cM = c.M, cWa = c.Wa, HaWa = c.Ha * c.Wa;
  const unsigned mul_hw = c.mul_hw, shr_hw = c.shr_hw, mul_w = c.mul_w, shr_w = c.shr_w;
  // every kernel-argument word the set-up needs is requested here, in one batch of scalar loads behind one wait,
  // instead of trickling in behind six dependent s_waitcnt round trips
  asm volatile("" ::"s"(ntaps), "s"(cM), "s"(cWa), "s"(HaWa), "s"(mul_hw), "s"(shr_hw), "s"(mul_w), "s"(shr_w),
               "s"(p.nwg_pad), "s"(p.tiles_n), "s"(p.tn_mul), "s"(p.tn_shr), "s"(p.Hin), "s"(p.Win), "s"(p.Cpix),
               "s"(p.Ktap), "s"(p.wt_row), "s"(p.sa), "s"(p.in), "s"(p.wt));
  // tap table in a VGPR (lane i = tap i) and fetched with v_readlane: the loops below index it dynamically, and a
  // scalar load per K-step would put an s_waitcnt lgkmcnt(0) — which also drains the LDS fragment reads — on the
  // critical path
  int tapv = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) tapv = (lane == i) ? taps_s[i] : tapv;

  const int bid = blockIdx.x;
  const int tile = (bid & 7) * (p.nwg_pad >> 3) + (bid >> 3);
  const int tile_m = fast_div(tile, p.tn_mul, p.tn_shr), tile_n = tile - tile_m * p.tiles_n;
  const int m0 = tile_m * BM;
  if (m0 >= cM) return;
  const int n0 = tile_n * BN;

  // ---- loader thread constants ----
  const int lrow = lane / CH, lchunk = lane % CH;
  const int ld_row = wave * RPI + lrow;                       // + it*RPI*NW
  const int src_chunk_el = (lchunk ^ swz_f<BK>(ld_row)) * 8;  // element offset of the 16B chunk this lane fetches
  // Per lane and tile row, everything that does not change over the K loop is computed once: the byte address of
  // the row's first channel chunk (tap (0,0)) and a bitmask of the taps that fall inside the image.  Per K-step
  // only a wave-uniform byte offset is added (tap displacement + channel chunk) — the gather costs ~6 VALU per row.
  const char* a_base[A_IT];
  unsigned a_valid[A_IT];
  const char* zero_src = (const char*)g_zero_page + src_chunk_el * 2;
#pragma unroll
  for (int it = 0; it < A_IT; ++it) {
    const int m = m0 + it * (RPI * NW) + ld_row;
    a_valid[it] = 0u;
    a_base[it] = zero_src;
    if (m < cM) {
      const int img = fast_div(m, mul_hw, shr_hw);
      const int rem = m - img * HaWa;
      const int a = fast_div(rem, mul_w, shr_w);
      const int b = rem - a * cWa;
      const int h0 = a * p.sa, w0 = b * p.sa;
      a_base[it] = (const char*)p.in + ((int64_t)((img * p.Hin + h0) * p.Win + w0) * p.Cpix + src_chunk_el) * 2;
      for (int ti = 0; ti < ntaps; ++ti) {   // wave-uniform trip count: one pass for a 1x1 conv
        const int tp = __builtin_amdgcn_readlane(tapv, ti);
        const int h = h0 + (tp & 0xff) - 64, w = w0 + ((tp >> 8) & 0xff) - 64;
        const unsigned ok = (((unsigned)h < (unsigned)p.Hin) & ((unsigned)w < (unsigned)p.Win)) ? 1u : 0u;
        a_valid[it] |= ok << ti;
      }
    }
  }
  // weight-tile swizzle: 8 distinct values over the even (and the odd) rows of {q*CPL + 4i + e}
  auto swz_w = [](int row) {
    if constexpr (!WIDE) return swz_f<BK>(row);
    else if constexpr (BK == 128) return (row & 3) | (((row / CPL) & 3) << 2);   // 16 distinct values over (q, e)
    else return ((row >> 1) & 1) | (((row / CPL) & 3) << 1);
  };
  unsigned b_off[B_IT];   // byte offset of this lane's chunk of weight row n (tap 0, k 0); fits 32 bits
#pragma unroll
  for (int it = 0; it < B_IT; ++it) {
    const int r = it * (RPI * NW) + ld_row;
    b_off[it] = (unsigned)(((int64_t)(n0 + r) * p.wt_row + (lchunk ^ swz_w(r)) * 8) * 2);
  }

  // grouped (ResNeXt) conv in block-diagonal form: weights carry 64 K-columns per tap — the 64 input channels of the
  // output tile's own channel block (zeros outside the true group) — so the K loop is one chunk per tap, read from
  // input-channel chunk n0 / 64
  const int kchunks = p.grouped ? 1 : p.Ktap / BK;
  const int in_kc0 = p.grouped ? n0 / BK : 0;
  const int T = ntaps * kchunks;
  const int Tg = KG == 1 ? T : (T + KG - 1) / KG;   // K-steps per group (shared barriers)
  // K order: channel chunk outermost, taps innermost.  All taps of a chunk touch the same input lines (shifted by
  // a pixel or a row), so within ~ntaps K-steps the workgroups of an XCD re-read a working set of
  // (pixels + halo) x 128 B instead of cycling through the whole (pixels x Cin) slab — the latter overflows the
  // 4 MB L2 for 256-channel 3x3 layers and drops the LDS-DMA stream to Infinity-Cache speed (~10 TB/s measured).
  int ld_tap = 0, ld_kc = 0;         // (tap, channel chunk) of the next K-step to be issued
  int ld_issued = grp;               // global index of the next K-step this group issues
  auto advance_k = [&]() {   // taps innermost
    if (++ld_tap == ntaps) { ld_tap = 0; ld_kc = (ld_kc + 1 == kchunks) ? 0 : ld_kc + 1; }
  };
  if constexpr (KG > 1) {
    for (int i = 0; i < grp; ++i) advance_k();
  }
  // issue the LDS-DMA of the next K-step into ring slot s (past the end: dummy loads of the zero page keep the
  // vmcnt bookkeeping uniform)
  auto stage_load = [&](int s) {
    char* sA = smem + s * STAGE + wave * (RPI * ROWB);
    char* sB = sA + A_BYTES;
    if (ld_issued < T) {
      ld_issued += KG;
      const int tp = __builtin_amdgcn_readlane(tapv, ld_tap);
      const int dh = (tp & 0xff) - 64, dw = ((tp >> 8) & 0xff) - 64, widx = tp >> 16;
      const int64_t uoff_a = ((int64_t)(dh * p.Win + dw) * p.Cpix + (ld_kc + in_kc0) * BK) * 2;   // wave-uniform
      const char* wt_u = (const char*)p.wt + ((int64_t)widx * p.Ktap + ld_kc * BK) * 2;  // wave-uniform
      const unsigned bit = 1u << ld_tap;
#pragma unroll
      for (int it = 0; it < A_IT; ++it) {
        const char* src = (a_valid[it] & bit) ? a_base[it] + uoff_a : zero_src;
        glds16(src, sA + it * (RPI * NW * ROWB));
      }
#pragma unroll
      for (int it = 0; it < B_IT; ++it) glds16(wt_u + b_off[it], sB + it * (RPI * NW * ROWB));
#pragma unroll
      for (int i = 0; i < KG; ++i) advance_k();
    } else {
#pragma unroll
      for (int it = 0; it < A_IT; ++it) glds16(zero_src, sA + it * (RPI * NW * ROWB));
#pragma unroll
      for (int it = 0; it < B_IT; ++it) glds16(zero_src, sB + it * (RPI * NW * ROWB));
    }
  };

  // ---- fragment reader constants ----
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 15, fq = lane >> 4;
  const int f_rd = swz_f<BK>(fr);
  int rd_off[KSUB];    // pixel-tile fragment j: sA + j*16*ROWB + rd_off[kk]
  int rdw_off[KSUB];   // weight-tile fragment i: sB + i*W_STEP + rdw_off[kk]
  constexpr int W_STEP = (WIDE ? 4 : 16) * ROWB;
  const int w_row0 = WIDE ? ((fr >> 2) * CPL + (fr & 3)) : fr;
  const int f_rd_w = !WIDE ? f_rd : (BK == 128 ? ((fr & 3) | ((fr >> 2) << 2)) : (((fr & 3) >> 1) | ((fr >> 2) << 1)));
#pragma unroll
  for (int kk = 0; kk < KSUB; ++kk) {
    rd_off[kk] = fr * ROWB + (((kk * 4 + fq) ^ f_rd) * 16);
    rdw_off[kk] = w_row0 * ROWB + (((kk * 4 + fq) ^ f_rd_w) * 16);
  }

  f32x4_t acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  auto mfma_substep = [&](const char* sA, const char* sB, int kk) {
    bf16x8_t wf[FN], xf[FM];
#pragma unroll
    for (int i = 0; i < FN; ++i) wf[i] = lds_read_b128(sB + i * W_STEP + rdw_off[kk]);
#pragma unroll
    for (int j = 0; j < FM; ++j) xf[j] = lds_read_b128(sA + j * 16 * ROWB + rd_off[kk]);
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j)
        acc[i][j] = mfma16<F16>(wf[i], xf[j], acc[i][j]);
  };

  // epilogue constants; with KG groups, fragment (i, j) is finished by group (i*FM + j) % KG
  // channel of (fragment i, register e) of this lane: ch_base + i*CH_STEP + e
  constexpr int CH_STEP = WIDE ? 4 : 16;
  const int ch_base = n0 + wn * WTN + fq * (WIDE ? CPL : 4);
  f32x4_t sc[FN], sh[FN];
  auto load_affine = [&]() {
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      sc[i] = p.scale ? *(const f32x4_t*)(p.scale + ch_base + i * CH_STEP) : (f32x4_t){1.f, 1.f, 1.f, 1.f};
      sh[i] = p.shift ? *(const f32x4_t*)(p.shift + ch_base + i * CH_STEP) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
  };
  if constexpr (EARLY_EPI) load_affine();   // older than every LDS-DMA: the counted vmcnt waits retire them first
  // Small tiles also fetch the epilogue's per-pixel operands here — the residual addend (same-size mode) and the ReLU
  // mask source of the lane's own outputs — so their latency runs beside the prologue's first-data latency instead
  // of behind the K loop (they are older than every LDS-DMA too).  Same values, same arithmetic order.
  // Only where the 16 extra registers cost no occupancy: the 64x64 4-wave tile (80 -> 96); the 128x128 8-wave tile would
  // cross 128 registers (two workgroups per CU -> one).
  constexpr bool PRE_EPI = EARLY_EPI && FN * FM <= 4 && WIDE && OWN_BY_J && KG == 1;
  bf16x8_t pre_add[PRE_EPI ? FM : 1][PRE_EPI ? FN / 2 : 1], pre_msk[PRE_EPI ? FM : 1][PRE_EPI ? FN / 2 : 1];
  const bool pre_have_add = PRE_EPI && p.addend_mode == TDN_ADD_SAME;
  const bool pre_have_msk = PRE_EPI && p.mask != nullptr;
  if constexpr (PRE_EPI) {
    if (pre_have_add || pre_have_msk) {
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        const int m = m0 + wm * WTM + j * 16 + fr;
        if (m < cM) {
          const int img = fast_div(m, mul_hw, shr_hw);
          const int rem = m - img * HaWa;
          const int a = fast_div(rem, mul_w, shr_w);
          const int b = rem - a * cWa;
          const int64_t opix = ((int64_t)img * p.Hout + (a * p.so + c.oh0)) * p.Wout + (b * p.so + c.ow0);
#pragma unroll
          for (int h = 0; h < FN / 2; ++h) {
            if (pre_have_add) pre_add[j][h] = *(const bf16x8_t*)(p.addend + opix * p.Cout + ch_base + h * 8);
            if (pre_have_msk) pre_msk[j][h] = *(const bf16x8_t*)(p.mask + opix * p.Cout + ch_base + h * 8);
          }
        }
      }
    }
  }

  if (Tg > 0) {
#pragma unroll
    for (int s = 0; s < NSTAGE - 1; ++s) stage_load(s);
    int slot = 0, fill = NSTAGE - 1;
    for (int t = 0; t < Tg; ++t) {
      wait_vm_and_barrier<LOADS * (NSTAGE - 2)>();   // K-step t has landed for every wave; slot (t-1) is free
      const char* sA = smem + slot * STAGE + (wm * WTM) * ROWB;
      const char* sB = smem + slot * STAGE + A_BYTES + (wn * WTN) * ROWB;
      if constexpr (MODE == 0) {
        stage_load(fill);
#pragma unroll
        for (int kk = 0; kk < KSUB; ++kk) mfma_substep(sA, sB, kk);
      } else if constexpr (MODE == 6) {
        // software-pipelined fragments: sub-step 1's LDS reads are issued between sub-step 0's MFMAs (second
        // register set), so only ONE LDS latency per K-step is exposed; the interleave is pinned with
        // sched_group_barrier (masks: 0x8 MFMA, 0x100 DS read, 0x20 VMEM read)
        static_assert(KSUB == 2, "pipelined-fragment schedule assumes BK = 64");
        bf16x8_t wf[2][FN], xf[2][FM];
#pragma unroll
        for (int i = 0; i < FN; ++i) wf[0][i] = lds_read_b128(sB + i * W_STEP + rdw_off[0]);
#pragma unroll
        for (int j = 0; j < FM; ++j) xf[0][j] = lds_read_b128(sA + j * 16 * ROWB + rd_off[0]);
        stage_load(fill);
#pragma unroll
        for (int i = 0; i < FN; ++i) wf[1][i] = lds_read_b128(sB + i * W_STEP + rdw_off[1]);
#pragma unroll
        for (int j = 0; j < FM; ++j) xf[1][j] = lds_read_b128(sA + j * 16 * ROWB + rd_off[1]);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j)
              acc[i][j] = mfma16<F16>(wf[kk][i], xf[kk][j], acc[i][j]);
        __builtin_amdgcn_sched_group_barrier(0x100, FN + FM, 0);
        __builtin_amdgcn_sched_group_barrier(0x20, LOADS, 0);
#pragma unroll
        for (int r = 0; r < FN + FM; ++r) {
          __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x8, 2 * FN * FM - (FN + FM), 0);
      } else {
        static_assert(MODE == 0, "unknown MODE");
      }
      slot = (slot + 1 == NSTAGE) ? 0 : slot + 1;
      fill = (fill + 1 == NSTAGE) ? 0 : fill + 1;
    }
    // drain the dummy tail loads before the LDS ring / registers are reused
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }

  // ---- split-K groups: exchange the partial accumulators through LDS (the rings are idle now) ----
  // layout: [group][wave][fragment][lane] x 16 B, conflict-free 16-byte accesses; summed in group order 0..KG-1 by
  // whichever group owns the fragment, so the result does not depend on the ownership map
  if constexpr (KG > 1) {
    __builtin_amdgcn_s_barrier();   // every wave is done reading the rings
    char* mine = smem_all + (((grp * NW + wave) * (FN * FM)) << 10) + lane * 16;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j) *(f32x4_t*)(mine + ((i * FM + j) << 10)) = acc[i][j];
    __syncthreads();
  }
  auto fragment = [&](int i, int j) -> f32x4_t {
    if constexpr (KG == 1) {
      return acc[i][j];
    } else {
      const char* src = smem_all + (((wave * (FN * FM)) + i * FM + j) << 10) + lane * 16;
      f32x4_t v = *(const f32x4_t*)src;
#pragma unroll
      for (int g = 1; g < KG; ++g) v += *(const f32x4_t*)(src + ((g * NW * (FN * FM)) << 10));
      return v;
    }
  };

  // ---- epilogue: per pixel fragment j the lane owns channels ch_base + i*CH_STEP + (0..3), i < FN ----
  if constexpr (!EARLY_EPI) load_affine();
#pragma unroll
  for (int j = 0; j < FM; ++j) {
    const int m = m0 + wm * WTM + j * 16 + fr;
    if (m >= cM) continue;
    const int img = fast_div(m, mul_hw, shr_hw);
    const int rem = m - img * HaWa;
    const int a = fast_div(rem, mul_w, shr_w);
    const int b = rem - a * cWa;
    const int oh = a * p.so + c.oh0, ow = b * p.so + c.ow0;
    const int64_t opix = ((int64_t)img * p.Hout + oh) * p.Wout + ow;
    int64_t apix = opix;
    if (p.addend_mode == TDN_ADD_UP2X)
      apix = ((int64_t)img * p.addend_h + (oh >> 1)) * p.addend_w + (ow >> 1);
    else if (p.addend_mode == TDN_ADD_SUMPOOL2)
      apix = ((int64_t)img * p.addend_h + 2 * oh) * p.addend_w + 2 * ow;
    if constexpr (WIDE && OWN_BY_J) {
      // ---- wide form: this lane's CPL consecutive channels of the pixel in one go ----
      if (KG > 1 && j % KG != grp) continue;
      f32x4_t v[FN];
#pragma unroll
      for (int i = 0; i < FN; ++i) v[i] = fragment(i, j) * sc[i] + sh[i];
      auto add_row = [&](const bf16_t* ap) {
#pragma unroll
        for (int h = 0; h < FN / 2; ++h) {
          const bf16x8_t r = *(const bf16x8_t*)(ap + h * 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[2 * h][e] += elem_to_f32<F16>(r[e]);
            v[2 * h + 1][e] += elem_to_f32<F16>(r[4 + e]);
          }
        }
      };
      if (p.addend_mode == TDN_ADD_SUMPOOL2) {
        // sum in a fixed order: (0,0) + (0,1) + (1,0) + (1,1)
        const bf16_t* ap = p.addend + apix * p.Cout + ch_base;
        const bf16_t* rows[4] = {ap, ap + p.Cout, ap + (int64_t)p.addend_w * p.Cout,
                                 ap + (int64_t)(p.addend_w + 1) * p.Cout};
#pragma unroll
        for (int h = 0; h < FN / 2; ++h) {
          float acc8[8];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bf16x8_t r = *(const bf16x8_t*)(rows[q] + h * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc8[e] = q == 0 ? elem_to_f32<F16>(r[e]) : acc8[e] + elem_to_f32<F16>(r[e]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[2 * h][e] += acc8[e]; v[2 * h + 1][e] += acc8[4 + e]; }
        }
      } else if (p.addend_mode != TDN_ADD_NONE) {
        if (pre_have_add) {
#pragma unroll
          for (int h = 0; h < FN / 2; ++h) {
            const bf16x8_t r = pre_add[PRE_EPI ? j : 0][PRE_EPI ? h : 0];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              v[2 * h][e] += elem_to_f32<F16>(r[e]);
              v[2 * h + 1][e] += elem_to_f32<F16>(r[4 + e]);
            }
          }
        } else {
          add_row(p.addend + apix * p.Cout + ch_base);
        }
      }
      if (p.relu) {
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[i][e] = fmaxf(v[i][e], 0.f);
        if (p.relu == 2) {
#pragma unroll
          for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = relu6_top<F16>(v[i][e]);
        }
      }
      if (p.mask) {
#pragma unroll
        for (int h = 0; h < FN / 2; ++h) {
          const bf16x8_t mk = pre_have_msk ? pre_msk[PRE_EPI ? j : 0][PRE_EPI ? h : 0]
                                           : *(const bf16x8_t*)(p.mask + opix * p.Cout + ch_base + h * 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[2 * h][e] = (elem_to_f32<F16>(mk[e]) > 0.f) ? v[2 * h][e] : 0.f;
            v[2 * h + 1][e] = (elem_to_f32<F16>(mk[4 + e]) > 0.f) ? v[2 * h + 1][e] : 0.f;
          }
        }
      }
      if (p.out_f32) {
#pragma unroll
        for (int i = 0; i < FN; ++i) *(f32x4_t*)((float*)p.out + opix * p.Cout + ch_base + i * 4) = v[i];
      } else {
#pragma unroll
        for (int h = 0; h < FN / 2; ++h) {
          bf16x8_t o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = f32_to_elem<F16>(v[2 * h][e]);
            o[4 + e] = f32_to_elem<F16>(v[2 * h + 1][e]);
          }
          *(bf16x8_t*)(p.out + opix * p.Cout + ch_base + h * 8) = o;
        }
      }
    } else {
  #pragma unroll
      for (int i = 0; i < FN; ++i) {
        if (KG > 1 && (i * FM + j) % KG != grp) continue;
        const int ch = ch_base + i * CH_STEP;
        f32x4_t v = fragment(i, j) * sc[i] + sh[i];
        if (p.addend_mode != TDN_ADD_NONE) {
          const bf16_t* ap = p.addend + apix * p.Cout + ch;
          const f32x4_t r = load4_f32<F16>(ap);
          if (p.addend_mode == TDN_ADD_SUMPOOL2) {
            // sum in a fixed order: (0,0) + (0,1) + (1,0) + (1,1)
            const f32x4_t r1 = load4_f32<F16>(ap + p.Cout);
            const f32x4_t r2 = load4_f32<F16>(ap + (int64_t)p.addend_w * p.Cout);
            const f32x4_t r3 = load4_f32<F16>(ap + (int64_t)(p.addend_w + 1) * p.Cout);
  #pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += ((r[e] + r1[e]) + r2[e]) + r3[e];
          } else {
            v += r;
          }
        }
        if (p.relu) {
  #pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
          if (p.relu == 2) {
  #pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = relu6_top<F16>(v[e]);
          }
        }
        if (p.mask) {
          const f32x4_t mk = load4_f32<F16>(p.mask + opix * p.Cout + ch);
  #pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (mk[e] > 0.f) ? v[e] : 0.f;
        }
        if (p.out_f32) {
          *(f32x4_t*)((float*)p.out + opix * p.Cout + ch) = v;
        } else {
          store4_f32<F16>(p.out + opix * p.Cout + ch, v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static inline void class_divisors(GemmClass& c) {
  fast_div_init((unsigned)(c.Ha * c.Wa), &c.mul_hw, &c.shr_hw);
  fast_div_init((unsigned)c.Wa, &c.mul_w, &c.shr_w);
}

// Tile configurations, one row per tile: X(id, BM, BN, BK, WM, WN, NSTAGE, MODE, TAG, KG).
// LDS = KG * NSTAGE * (BM + BN) * BK * 2 bytes.  These seven are the set choose_cfg picks from, built for both element
// types; the library also holds the TAG-1 twin of 3 and the stem's 128x64x32.  kCfgs[] (the planner's and
// tdn_conv2d_plan's view) and the switches of dispatch_gemm (the instantiations) are both generated from this list.
// The ids are names, not row numbers: the tests, DESIGN.md and every recorded profile use them, and the gaps are the
// alternate tiles, timing-only ablations and cycle-stamp builds that were measured and dropped.
// MODE 0: LDS-DMA of the next K-step right after the barrier, fragments read per sub-step; MODE 6: fragment reads
// software-pipelined under the MFMAs.
#define TDN_GEMM_CFGS(X) \
  X(0, 64, 64, 64, 2, 2, 2, 0, 0, 1)     /* 32 KB, 256 thr: Cout = 64 layers, tiny grids */                                \
  X(1, 64, 128, 64, 2, 2, 2, 6, 0, 1)    /* 48 KB, 256 thr: mid-size layers */                                             \
  X(2, 128, 128, 64, 2, 2, 2, 6, 0, 1)   /* 64 KB, 256 thr: large-M, Cout = 128 */                                         \
  X(3, 192, 256, 64, 2, 4, 2, 6, 0, 1)   /* 112 KB, 512 thr: large-M, Cout % 256 == 0 (fewest L2->LDS bytes per flop) */   \
  X(25, 64, 64, 64, 2, 2, 2, 0, 0, 2)    /* in-workgroup split-K: 2 groups x 4 waves, 64 KB */                             \
  X(46, 128, 128, 64, 2, 4, 2, 6, 0, 1)  /* 8 waves, 64 KB: mid-size layers with >= 128 such tiles */                      \
  X(50, 64, 64, 128, 2, 2, 2, 0, 0, 1)   /* BK = 128: twice the work per ~1300-cycle K-step */
struct GemmCfg { int id, bm, bn, bk, wm, wn, nstage, mode, tag, kg; };
#define TDN_CFG_ROW(id, bm, bn, bk, wm, wn, nstage, mode, tag, kg) {id, bm, bn, bk, wm, wn, nstage, mode, tag, kg},
static const GemmCfg kCfgs[] = {TDN_GEMM_CFGS(TDN_CFG_ROW)};

// the row named `id`, or nullptr
static const GemmCfg* find_cfg(int id) {
  for (const GemmCfg& t : kCfgs)
    if (t.id == id) return &t;
  return nullptr;
}

// a forced generic tile (tests, sweeps) is in effect: it also keeps the conv away from the halo kernel.  An empty
// value counts and reads as config 0.
static bool gemm_cfg_forced() { return tdn_knob_present("TDN_GEMM_CFG") != nullptr; }

static int choose_cfg(int maxM, int ngemm, int kgemm, int grouped = 0, int ktap = 64) {
  if (grouped) return 0;   // block-diagonal grouped conv: one 64-channel block per N tile
  if (gemm_cfg_forced()) {
    const GemmCfg* t = find_cfg(tdn_knob_int("TDN_GEMM_CFG", 0));
    if (t && ngemm % t->bn == 0 && ktap % t->bk == 0) return t->id;
  }
  // sweep-only overrides of the thresholds below; a set but empty value reads as 0
  auto sweep = [](const char* name, int dflt) { return tdn_knob_present(name) ? tdn_knob_int(name, 0) : dflt; };
  // Measured on MI355X over the R50-FPN shapes (scripts/conv_bench.py; profiles/convbench_*.log): several small
  // co-resident workgroups per CU (64-pixel tiles, 2-deep ring, 32-48 KB LDS) beat one large deeply pipelined
  // workgroup on almost every shape; only the very large-M 3x3 convs prefer the 256x128 8-wave tile.
  const int big_minm = sweep("TDN_T192_MINM", 24000);
  if (ngemm % 256 == 0 && maxM >= big_minm) return 3;   // 192x256, 8 waves: fewest L2->LDS bytes per flop
  // few tiles and a long K loop (layer4, the top FPN levels): every CU holds at most two 4-wave workgroups and the
  // LDS-DMA stream starves (~4 B/clk per loading wave) — recruit a second wave group along K (in-workgroup split-K).
  // Cutting K over several workgroups with an exchange through memory lost to the unsplit tiles on every such layer
  // (layer4 3x3: 28 us unsplit, 32 / 37 us XCD-local / agent scope): it multiplies the per-workgroup fixed cost.
  const int kg_tiles = sweep("TDN_KG_TILES", 512);
  const int kg_kmin = sweep("TDN_KG_KMIN", 2048);
  if ((long)ceil_div(maxM, 64) * (ngemm / 64) <= kg_tiles && kgemm >= kg_kmin) return 25;
  // at most about one 64x64 tile per CU and a K loop of 16-31 steps (layer3's 1024 -> 256 convs and the dgrad of its
  // 256 -> 1024 ones, per image: 264 tiles): 128-deep K-steps halve the barriers of a workgroup that has its CU to
  // itself.  Whole-step A/B on one box, three interleaved pairs: +0.6-0.9 %; the same tile on the neighbouring shapes
  // (528 tiles, or K = 512, or K = 2048 where the K groups above already apply) is neutral to -0.7 %.
  const int bk128_tiles = sweep("TDN_BK128_TILES", 300);
  // 1x1 convs only: with several taps a 128-deep chunk changes the (chunk outer, taps inner) summation order
  if (kgemm == ktap && (long)ceil_div(maxM, 64) * (ngemm / 64) <= bk128_tiles && kgemm >= 1024 && ktap % 128 == 0)
    return 50;
  if (ngemm % 128 == 0) {
    // A K-step costs ~1300-1500 cycles of load latency whatever the tile (cycle stamps), so the 128x128
    // tile does 2-4x the work per step of the 64-wide ones; with 8 waves (wave tile 64x32) two of them fit a CU.
    // Alone on the GPU it wins from ~128 tiles up, but inside the step (side-stream wgrad kernels beside the dgrad
    // chain) the 132-tile layers of layer3 (M = 8400, N = 256) run faster as 528 64x64 workgroups: whole-step A/B on
    // one box, threshold 128 -> 396 img/s, 140..200 -> 402, 268 and up -> 395 and falling.  The thresholds are
    // overridable (TDN_T128_MIN, TDN_T64_MIN, TDN_KG_TILES, TDN_KG_KMIN, TDN_T192_MINM) for such sweeps.
    const int t128_min = sweep("TDN_T128_MIN", 200);
    const int t64_min = sweep("TDN_T64_MIN", 300);
    if ((long)ceil_div(maxM, 128) * (ngemm / 128) >= t128_min) return 46;
    const long t64 = (long)ceil_div(maxM, 64) * (ngemm / 128);
    return t64 >= t64_min ? 1 : 0;
  }
  return 0;
}

template <int BM, int BN, int BK, int WM, int WN, int NSTAGE, int MODE = 0, int TAG = 0, int KG = 1, bool F16 = false>
static int launch_gemm(GemmParams& p, int maxM, hipStream_t stream) {
  p.tiles_n = p.Cout / BN;
  fast_div_init((unsigned)p.tiles_n, &p.tn_mul, &p.tn_shr);
  const int ntiles = ceil_div(maxM, BM) * p.tiles_n;
  p.nwg_pad = (ntiles + 7) & ~7;
  constexpr size_t lds = (size_t)KG * NSTAGE * (BM + BN) * BK * 2;
  const int first =
      tdn_allow_lds<conv_gemm_kernel<BM, BN, BK, WM, WN, NSTAGE, MODE, TAG, KG, F16>>((int)lds, "conv_gemm");
  if (first < 0) return first;
  if (first && tdn_knob_present("TDN_DEBUG_OCC")) {
    int nb = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &nb, (const void*)conv_gemm_kernel<BM, BN, BK, WM, WN, NSTAGE, MODE, TAG, KG, F16>, WM * WN * KG * 64, lds);
    fprintf(stderr, "[tdn] conv_gemm<%d,%d,%d,%d,%d,%d,%d,%d,%d,%s>: %d B LDS, %d workgroups/CU\n", BM, BN, BK, WM,
            WN, NSTAGE, MODE, TAG, KG, F16 ? "f16" : "bf16", (int)lds, nb);
  }
  dim3 grid(p.nwg_pad, p.ncls, 1), block(WM * WN * KG * 64, 1, 1);
  TDN_LAUNCH((conv_gemm_kernel<BM, BN, BK, WM, WN, NSTAGE, MODE, TAG, KG, F16>), grid, block, lds, stream, p);
  TDN_LAUNCH_CHECK();
  return 0;
}

// Tile `ID` of TDN_GEMM_CFGS.
template <int ID, int BM, int BN, int BK, int WM, int WN, int NSTAGE, int MODE, int TAG, int KG, bool F16>
static int launch_cfg(GemmParams& p, int maxM, hipStream_t stream) {
  if constexpr (ID == 3 && !F16) {
    // TDN_TAG_DOMINANT (set by bench.py around exactly the launches it brackets with HIP events): same code under
    // the TAG-1 symbol, so rocprofv3 --stats lists those launches on a line of their own
    if (maxM >= 100000 && p.Cout == 256 && p.cls[0].ntaps * p.Ktap == 2304 && tdn_knob_present("TDN_TAG_DOMINANT"))
      return launch_gemm<BM, BN, BK, WM, WN, NSTAGE, MODE, 1, KG, F16>(p, maxM, stream);
  }
  return launch_gemm<BM, BN, BK, WM, WN, NSTAGE, MODE, TAG, KG, F16>(p, maxM, stream);
}

// switch cases from TDN_GEMM_CFGS, in table order: it is the order in which the compiler emits the kernels, so the
// code object can be compared with an older build section by section
#define TDN_CFG_CASE(id, bm, bn, bk, wm, wn, nstage, mode, tag, kg) \
  case id: return launch_cfg<id, bm, bn, bk, wm, wn, nstage, mode, tag, kg, F16>(p, maxM, stream);

static int dispatch_gemm(GemmParams& p, int maxM, hipStream_t stream, int dtype) {
  if (maxM <= 0) return 0;
  const int id = choose_cfg(maxM, p.Cout, p.cls[0].ntaps * p.Ktap, p.grouped, p.Ktap);
  if (dtype == TDN_F16) {
    constexpr bool F16 = true;
    switch (id) {
      TDN_GEMM_CFGS(TDN_CFG_CASE)
      default: TDN_CHECK(false, "bad GEMM config id"); return -1;
    }
  }
  constexpr bool F16 = false;
  switch (id) {
    TDN_GEMM_CFGS(TDN_CFG_CASE)
    default: TDN_CHECK(false, "bad GEMM config id"); return -1;
  }
}

static int check_conv_shape(int N, int H, int W, int Cin, int Cout, int k, int stride, int pad, int dtype) {
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(N > 0 && H > 0 && W > 0, "bad tensor shape N=%d H=%d W=%d", N, H, W);
  if (conv_check_rules(k, stride, pad, Cin, Cout)) return -1;
  TDN_CHECK((int64_t)N * H * W < (1ll << 31) / 4, "tensor too large for 32-bit pixel indexing");
  return 0;
}

static void build_fwd(GemmParams& p, int N, int H, int W, int Cin, int Cout, int k, int stride, int pad) {
  const int Ho = conv_out_sz(H, k, stride, pad), Wo = conv_out_sz(W, k, stride, pad);
  const int d = conv_dil(k, pad);
  p.Hin = H; p.Win = W; p.Cpix = Cin; p.Ktap = Cin; p.wt_row = k * k * Cin;
  p.Hout = Ho; p.Wout = Wo; p.Cout = Cout; p.sa = stride; p.so = 1; p.ncls = 1; p.grouped = 0;
  GemmClass& c = p.cls[0];
  c.Ha = Ho; c.Wa = Wo; c.M = N * Ho * Wo; c.oh0 = 0; c.ow0 = 0; c.ntaps = 0;
  for (int kh = 0; kh < k; ++kh)
    for (int kw = 0; kw < k; ++kw) c.taps[c.ntaps++] = pack_tap(kh * d - pad, kw * d - pad, kh * k + kw);
  class_divisors(c);
}

// Input gradient as a gather: dx[hi][wi] = sum over (kh,kw) with (hi+pad-kh) % s == 0 of g[(hi+pad-kh)/s] * w[kh][kw].
static int build_dgrad(GemmParams& p, int N, int H, int W, int Cin, int Cout, int k, int stride, int pad) {
  const int Ho = conv_out_sz(H, k, stride, pad), Wo = conv_out_sz(W, k, stride, pad);
  const int d = conv_dil(k, pad);
  p.Hin = Ho; p.Win = Wo; p.Cpix = Cout; p.Ktap = Cout; p.wt_row = k * k * Cout;
  p.Hout = H; p.Wout = W; p.Cout = Cin; p.sa = 1; p.so = stride; p.grouped = 0;
  p.ncls = stride * stride;
  int maxM = 0;
  for (int ph = 0; ph < stride; ++ph)
    for (int pw = 0; pw < stride; ++pw) {
      GemmClass& c = p.cls[ph * stride + pw];
      c.Ha = (H - ph + stride - 1) / stride;
      c.Wa = (W - pw + stride - 1) / stride;
      if (c.Ha < 0) c.Ha = 0;
      if (c.Wa < 0) c.Wa = 0;
      c.M = N * c.Ha * c.Wa;
      c.oh0 = ph; c.ow0 = pw; c.ntaps = 0;
      for (int kh = 0; kh < k; ++kh) {
        if ((ph + pad - kh * d) % stride != 0) continue;
        for (int kw = 0; kw < k; ++kw) {
          if ((pw + pad - kw * d) % stride != 0) continue;
          // floor division (the numerator is negative for large dilations): it is an exact multiple of stride
          c.taps[c.ntaps++] = pack_tap((ph + pad - kh * d) / stride, (pw + pad - kw * d) / stride, kh * k + kw);
        }
      }
      class_divisors(c);
      if (c.M > maxM) maxM = c.M;
    }
  return maxM;
}

extern "C" int tdn_conv2d_fwd(const void* x, const void* w_fwd, void* y, int N, int H, int W, int Cin,
                              int Cout, int k, int stride, int pad, const tdn_epilogue* ep, int dtype,
                              void* stream) {
  if (check_conv_shape(N, H, W, Cin, Cout, k, stride, pad, dtype)) return -1;
  TDN_CHECK(x && w_fwd && y, "tdn_conv2d_fwd: NULL tensor pointer");
  GemmParams p;
  build_fwd(p, N, H, W, Cin, Cout, k, stride, pad);
  p.in = (const bf16_t*)x; p.wt = (const bf16_t*)w_fwd; p.out = (bf16_t*)y;
  if (conv_fill_epilogue(p, ep, p.Hout, p.Wout)) return -1;
  if (!gemm_cfg_forced()) {
    const int h = tdn_halo_conv_fwd(x, w_fwd, y, N, H, W, Cin, Cout, k, stride, pad, ep, dtype, (hipStream_t)stream);
    if (h != 0) return h < 0 ? h : 0;
  }
  return dispatch_gemm(p, p.cls[0].M, (hipStream_t)stream, dtype);
}

extern "C" int tdn_conv2d_dgrad(const void* g, const void* w_dgrad, void* dx, int N, int H, int W, int Cin,
                                int Cout, int k, int stride, int pad, const tdn_epilogue* ep, int dtype,
                                void* stream) {
  if (check_conv_shape(N, H, W, Cin, Cout, k, stride, pad, dtype)) return -1;
  TDN_CHECK(g && w_dgrad && dx, "tdn_conv2d_dgrad: NULL tensor pointer");
  GemmParams p;
  const int maxM = build_dgrad(p, N, H, W, Cin, Cout, k, stride, pad);
  p.in = (const bf16_t*)g; p.wt = (const bf16_t*)w_dgrad; p.out = (bf16_t*)dx;
  if (conv_fill_epilogue(p, ep, p.Hout, p.Wout)) return -1;
  if (!gemm_cfg_forced()) {
    const int h = tdn_halo_conv_dgrad(g, w_dgrad, dx, N, H, W, Cin, Cout, k, stride, pad, ep, dtype,
                                      (hipStream_t)stream);
    if (h != 0) return h < 0 ? h : 0;
  }
  return dispatch_gemm(p, maxM, (hipStream_t)stream, dtype);
}

// Grouped 3x3 / 1x1 conv (ResNeXt, models/backbone/resnext.py:26-28,82-83: conv3x3_group(..., groups=cardinality)) in
// block-diagonal form: C channels in and out, C % 64 == 0, channels per group dividing 64.  Operands come from
// tdn_pack_gconv_weight ([C][k][k][64]); every 64-channel output block multiplies only its own 64 input channels.
static int check_gconv(int C, int groups) {
  TDN_CHECK(groups > 0 && C % groups == 0, "grouped conv: %d groups do not divide %d channels", groups, C);
  const int cpg = C / groups;
  TDN_CHECK(C % 64 == 0 && cpg <= 64 && 64 % cpg == 0,
            "grouped conv: need C %% 64 == 0 and channels per group dividing 64 (C=%d, groups=%d)", C, groups);
  return 0;
}

extern "C" int tdn_gconv2d_fwd(const void* x, const void* w_fwd, void* y, int N, int H, int W, int C, int groups,
                               int k, int stride, int pad, const tdn_epilogue* ep, int dtype, void* stream) {
  if (check_conv_shape(N, H, W, C, C, k, stride, pad, dtype) || check_gconv(C, groups)) return -1;
  TDN_CHECK(x && w_fwd && y, "tdn_gconv2d_fwd: NULL tensor pointer");
  GemmParams p;
  build_fwd(p, N, H, W, C, C, k, stride, pad);
  p.grouped = 1; p.Ktap = 64; p.wt_row = k * k * 64;
  p.in = (const bf16_t*)x; p.wt = (const bf16_t*)w_fwd; p.out = (bf16_t*)y;
  if (conv_fill_epilogue(p, ep, p.Hout, p.Wout)) return -1;
  return dispatch_gemm(p, p.cls[0].M, (hipStream_t)stream, dtype);
}

extern "C" int tdn_gconv2d_dgrad(const void* g, const void* w_dgrad, void* dx, int N, int H, int W, int C, int groups,
                                 int k, int stride, int pad, const tdn_epilogue* ep, int dtype, void* stream) {
  if (check_conv_shape(N, H, W, C, C, k, stride, pad, dtype) || check_gconv(C, groups)) return -1;
  TDN_CHECK(g && w_dgrad && dx, "tdn_gconv2d_dgrad: NULL tensor pointer");
  GemmParams p;
  const int maxM = build_dgrad(p, N, H, W, C, C, k, stride, pad);
  p.grouped = 1; p.Ktap = 64; p.wt_row = k * k * 64;
  p.in = (const bf16_t*)g; p.wt = (const bf16_t*)w_dgrad; p.out = (bf16_t*)dx;
  if (conv_fill_epilogue(p, ep, p.Hout, p.Wout)) return -1;
  return dispatch_gemm(p, maxM, (hipStream_t)stream, dtype);
}

// Stem: 7x7 s2 p3 conv on the zero-padded NHWC4 staging buffer xp[N][H+6][W+8][4]. One "tap" per kernel
// row kh: 8 consecutive pixels x 4 channels = 32 contiguous bf16 (kw = 7 and c = 3 carry zero weights).
extern "C" int tdn_stem_conv_fwd(const void* xp, const void* w_stem, void* y, int N, int H, int W, int Cout,
                                 const tdn_epilogue* ep, int dtype, void* stream) {
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(xp && w_stem && y, "tdn_stem_conv_fwd: NULL tensor pointer");
  TDN_CHECK(H % 2 == 0 && W % 2 == 0 && H > 0 && W > 0 && N > 0, "stem needs even H, W (got %dx%d)", H, W);
  TDN_CHECK(Cout % 64 == 0, "stem Cout must be a multiple of 64");
  GemmParams p;
  const int Ho = H / 2, Wo = W / 2;
  p.Hin = H + 6; p.Win = W + 8; p.Cpix = 4; p.Ktap = 32; p.wt_row = 7 * 32;
  p.Hout = Ho; p.Wout = Wo; p.Cout = Cout; p.sa = 2; p.so = 1; p.ncls = 1; p.grouped = 0;
  GemmClass& c = p.cls[0];
  c.Ha = Ho; c.Wa = Wo; c.M = N * Ho * Wo; c.oh0 = 0; c.ow0 = 0; c.ntaps = 7;
  for (int kh = 0; kh < 7; ++kh) c.taps[kh] = pack_tap(kh, 0, kh);
  class_divisors(c);
  p.in = (const bf16_t*)xp; p.wt = (const bf16_t*)w_stem; p.out = (bf16_t*)y;
  if (conv_fill_epilogue(p, ep, Ho, Wo)) return -1;
  if (dtype == TDN_F16) return launch_gemm<128, 64, 32, 2, 2, 3, 0, 0, 1, true>(p, c.M, (hipStream_t)stream);
  return launch_gemm<128, 64, 32, 2, 2, 3>(p, c.M, (hipStream_t)stream);
}

extern "C" int tdn_conv2d_plan(int kind, int N, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                               int32_t* out16);
int tdn_wgrad_plan(int N, int H, int W, int Cin, int Cout, int k, int stride, int pad, int32_t* out16);

extern "C" int tdn_conv2d_plan(int kind, int N, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                               int32_t* o) {
  if (check_conv_shape(N, H, W, Cin, Cout, k, stride, pad, TDN_BF16)) return -1;
  TDN_CHECK(o != nullptr, "tdn_conv2d_plan: NULL output");
  for (int i = 0; i < 16; ++i) o[i] = 0;
  if (kind == 2) return tdn_wgrad_plan(N, H, W, Cin, Cout, k, stride, pad, o);
  TDN_CHECK(kind == 0 || kind == 1, "tdn_conv2d_plan: bad kind %d", kind);
  GemmParams p;
  int maxM;
  if (kind == 0) { build_fwd(p, N, H, W, Cin, Cout, k, stride, pad); maxM = p.cls[0].M; }
  else maxM = build_dgrad(p, N, H, W, Cin, Cout, k, stride, pad);
  const GemmCfg& t = *find_cfg(choose_cfg(maxM, p.Cout, p.cls[0].ntaps * p.Ktap, p.grouped, p.Ktap));
  int Mtot = 0, taps_tot = 0;
  for (int i = 0; i < p.ncls; ++i) { Mtot += p.cls[i].M; taps_tot += p.cls[i].ntaps; }
  o[0] = Mtot; o[1] = p.Cout; o[2] = p.cls[0].ntaps * p.Ktap; o[3] = t.bm; o[4] = t.bn; o[5] = t.bk;
  o[6] = (ceil_div(maxM, t.bm) * (p.Cout / t.bn) + 7) & ~7; o[7] = p.ncls; o[8] = 1; o[9] = p.ncls;
  o[10] = p.cls[0].ntaps; o[11] = 1; o[12] = taps_tot; o[13] = p.Hout; o[14] = p.Wout; o[15] = maxM;
  if (!gemm_cfg_forced()) (void)tdn_halo_plan(kind, N, H, W, Cin, Cout, k, stride, pad, o);   // o[8] >= 100: halo kernel
  return 0;
}
