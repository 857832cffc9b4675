// Fully connected layers: one MFMA GEMM family for the box head's linear layers.
//
//   forward   y[M][O]  = act(x[M][K] . w_fwd[Op][K]^T + bias)            linear_gemm_kernel, both operands K-contiguous
//   dgrad     dx[M][K] = mask(g[M][Op] . w_dgrad[K][Op]^T)               the same kernel: the reduction runs over Op
//   wgrad     dw[O][K] = beta * dw + g^T . x,  dbias = beta * dbias + column sums of g
//                                                                        linear_wgrad_kernel: the reduction runs over the
//                                                                        M rows, both operands are read transposed
//                                                                        (ds_read_b64_tr_b16)
//
// All three stage 64-deep steps of both operands into a two-slot LDS ring by LDS-DMA (16 bytes per lane; the XOR swizzle
// is applied to the SOURCE address and again to the read address) and accumulate in fp32 with mfma16<F16>.  A product
// whose tiles underfill the chip is cut along its reduction into slices of whole 64-element chunks: every workgroup then
// stores an fp32 partial slab into the caller's workspace with plain stores and a second, finalize launch sums the slabs
// in slice order, applies the epilogue and rounds once.  No workgroup waits for another one, there are no counters, no
// atomics and no memset: the result is the same bits on every run.
//
// Routing (the acceptance rule of the benchmark): with splits = 0, an UNSPLIT forward or input gradient of a
// layer whose O is a multiple of 64 is handed to tdn_conv2d_fwd / tdn_conv2d_dgrad as a 1x1 conv over M pixels — the conv
// GEMM's smaller tiles measured faster there (fc7, fc6's dgrad), and the two packs are the same bytes.  This file's
// kernel keeps the split forward (fc6), every ragged O (the predictors), every forced slice count and every weight
// gradient.
//
// A cotangent whose rows are not 16-byte aligned (the predictors' 81 / 324 / 405 columns) is first copied, zero padded
// to Op = O rounded up to 64 columns, into the workspace by one pad launch (linear_pad_kernel).
// Tiles, ring, swizzles, MFMA loops, split rule and plan record: csrc/gemm128_core.h, shared with csrc/deconv.hip.
#include "gemm128_core.h"

namespace {

constexpr int MAX_M = 1 << 18, MAX_O = 65536, MAX_K = 1 << 20;

// ---- forward / dgrad: C[m][n] = sum_k A[m][k] * B[n][k] -----------------------------------------------------------------
struct GemmArgs {
  const bf16_t* A; int64_t lda; int a_rows;   // rows m >= a_rows are read from the zero page
  const bf16_t* B; int64_t ldb; int b_rows;   // likewise rows n >= b_rows
  int M, N;                                   // extent of the output: nothing is stored at m >= M or n >= N
  int nchunks, cps, tiles_n, ntiles;          // reduction chunks of BK, chunks per slice
  void* out; int64_t ldo; int out_f32;        // one slice: the epilogue is applied here
  const float* bias; int relu;
  const bf16_t* mask; int64_t ldmask;
  int vec;                                    // out, mask rows allow 4-element vector access
  float* slab; int64_t slab_ld;               // more than one slice: slab[slice][M][slab_ld]
};

template <bool F16>
__device__ __forceinline__ void store_out(const GemmArgs& p, int64_t m, int n, float v) {
  if (p.bias) v += p.bias[n];
  if (p.relu) v = fmaxf(v, 0.f);
  if (p.mask && !(elem_to_f32<F16>(p.mask[m * p.ldmask + n]) > 0.f)) v = 0.f;
  if (p.out_f32) ((float*)p.out)[m * p.ldo + n] = v;
  else ((bf16_t*)p.out)[m * p.ldo + n] = f32_to_elem<F16>(v);
}

template <bool F16>
__global__ __launch_bounds__(NT) void linear_gemm_kernel(const GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slice = (int)blockIdx.x / p.ntiles, tile = (int)blockIdx.x - slice * p.ntiles;
  const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int c_begin = slice * p.cps, c_end = min(p.nchunks, c_begin + p.cps);

  // ---- loader: plain rows; a row past its operand reads the zero page
  const int lrow = lane >> 3;
  const int src_el = kc_src_el(lane, lrow);
  const bf16_t* const zero = (const bf16_t*)g_zero_page + src_el;
  const bf16_t* a_src[4];
  const bf16_t* b_src[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = kc_row(it, wave, lrow);
    a_src[it] = (m0 + row < p.a_rows) ? p.A + (int64_t)(m0 + row) * p.lda + src_el : nullptr;
    b_src[it] = (n0 + row < p.b_rows) ? p.B + (int64_t)(n0 + row) * p.ldb + src_el : nullptr;
  }
  auto stage_load = [&](int chunk, int s) {
    char* sA = smem + s * STAGE;
    char* sB = sA + TILE_BYTES;
    const int k0 = chunk * BK;
    const bool in = chunk < c_end;                  // past the slice: the zero page (keeps the vmcnt bookkeeping uniform)
#pragma unroll
    for (int it = 0; it < 4; ++it) glds16_async((in && a_src[it]) ? a_src[it] + k0 : zero, sA + kc_dst(it, wave));
#pragma unroll
    for (int it = 0; it < 4; ++it) glds16_async((in && b_src[it]) ? b_src[it] + k0 : zero, sB + kc_dst(it, wave));
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[4], b_off[4], k_off[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a_off[i] = kc_a_off(wm, i, fr);
    b_off[i] = kc_b_off(wn, i, fr);
  }
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) k_off[kk] = kc_k_off(kk, fq, fr);

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // kc_ring's loop, kept as this kernel's own text: through kc_ring the same instructions come out in another order,
  // which measured 4 % (split fc6) to 14 % (unsplit fc6) slower (profiles/gemm128_core_refactor_checks.md §4)
  if (c_end > c_begin) {
#pragma unroll
    for (int s = 0; s < NST - 1; ++s) stage_load(c_begin + s, s);
    int slot = 0, fill = NST - 1;
    for (int c = c_begin; c < c_end; ++c) {
      wait_step_and_barrier();                      // step c has landed for every wave; the slot of step c - 1 is free
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

  // ---- store ----
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wm * 64 + i * 16 + fr;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fq * 4;
      if (p.slab) {
        if (n < p.slab_ld) *(f32x4_t*)(p.slab + ((int64_t)slice * p.M + m) * p.slab_ld + n) = acc[i][j];
        continue;
      }
      if (n >= p.N) continue;
      if (p.vec && n + 3 < p.N) {
        f32x4_t v = acc[i][j];
        if (p.bias) v += *(const f32x4_t*)(p.bias + n);
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        if (p.mask) {
          const f32x4_t ms = load4_f32<F16>(p.mask + m * p.ldmask + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = ms[e] > 0.f ? v[e] : 0.f;
        }
        if (p.out_f32) *(f32x4_t*)((float*)p.out + m * p.ldo + n) = v;
        else store4_f32<F16>((bf16_t*)p.out + m * p.ldo + n, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < p.N) store_out<F16>(p, m, n + e, acc[i][j][e]);
      }
    }
  }
}

// out[m][n] = epilogue(sum over slices, in slice order, of slab[s][m][n])
template <bool F16>
__global__ __launch_bounds__(NT) void linear_finalize_kernel(const GemmArgs p, int slices) {
  const int64_t total = (int64_t)p.M * p.N;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    const int64_t m = idx / p.N;
    const int n = (int)(idx - m * p.N);
    const float* s = p.slab + m * p.slab_ld + n;
    const int64_t step = (int64_t)p.M * p.slab_ld;
    float v = s[0];
    for (int k = 1; k < slices; ++k) v += s[k * step];
    store_out<F16>(p, m, n, v);
  }
}

// gp[m][0..Op) = g[m][0..O), zeros behind: a 16-byte aligned, 64-column padded copy of a ragged cotangent
__global__ __launch_bounds__(NT) void linear_pad_kernel(const bf16_t* __restrict__ g, int64_t ldg, bf16_t* __restrict__ gp,
                                                        int M, int O, int Op) {
  const int64_t total = (int64_t)M * Op;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    const int64_t m = idx / Op;
    const int o = (int)(idx - m * Op);
    unsigned short v = 0;
    if (o < O) v = ((const unsigned short*)g)[m * ldg + o];
    ((unsigned short*)gp)[idx] = v;
  }
}

// out[m][o] = y[m][o] > 0 ? g[m][o] : 0: the cotangent behind a layer's own ReLU, read from its stored output (16-bit, or
// fp32 with y_f32).  Contiguous (M, O) operands; any O.
template <bool F16>
__global__ __launch_bounds__(NT) void linear_relu_bwd_kernel(const bf16_t* __restrict__ g, const void* __restrict__ y,
                                                             int y_f32, bf16_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    const float t = y_f32 ? ((const float*)y)[i] : elem_to_f32<F16>(((const bf16_t*)y)[i]);
    out[i] = t > 0.f ? g[i] : f32_to_elem<F16>(0.f);
  }
}

// ---- wgrad: dw[o][k] = sum_m g[m][o] * x[m][k] -----------------------------------------------------------------------
struct WgradArgs {
  const bf16_t* g; int64_t ldg; int g_cols;   // 16-byte pieces at columns >= g_cols come from the zero page
  const bf16_t* x; int64_t ldx;
  int M, O, K, C, hw;                         // hw == 1: columns as they are; else packed column p * C + c is logical c * hw + p
  int mchunks, cps, tiles_o, ntiles;
  float* dw; float* dbias; float beta;
  float* slab; float* colsum;                 // more than one slice: slab[slice][O][K] in PACKED column order
};

template <bool F16>
__global__ __launch_bounds__(NT) void linear_wgrad_kernel(const WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slice = (int)blockIdx.x / p.ntiles, tile = (int)blockIdx.x - slice * p.ntiles;
  const int tk = tile / p.tiles_o, to = tile - tk * p.tiles_o;
  const int o0 = to * BM, k0 = tk * BN;
  const int m_begin = slice * p.cps * BK;
  const int m_end = min(p.M, m_begin + p.cps * BK);

  // ---- loader: plain rows; a piece at a column past its operand and a row >= m_end read the zero page
  const int lrow = lane >> 4, pc = lane & 15;
  const int row0 = tr_row0(wave, lrow);         // + it * 16
  const int src_el = tr_src_el(pc, row0);
  const bf16_t* const zero = (const bf16_t*)g_zero_page + (src_el & 63);
  const bool g_ok = o0 + src_el < p.g_cols, x_ok = k0 + src_el < p.K;
  const bf16_t* const gsrc = p.g + o0 + src_el;
  const bf16_t* const xsrc = p.x + k0 + src_el;
  auto stage_load = [&](int mt, int s) {
    char* sG = smem + s * STAGE;
    char* sX = sG + TILE_BYTES;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int m = mt + it * 16 + row0;
      glds16_async((g_ok && m < m_end) ? gsrc + (int64_t)m * p.ldg : zero, sG + tr_dst(it, wave));
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int m = mt + it * 16 + row0;
      glds16_async((x_ok && m < m_end) ? xsrc + (int64_t)m * p.ldx : zero, sX + tr_dst(it, wave));
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int grp4 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int rrow = 8 * grp4 + q;                // + kk * 32 + 4 * half
  const int f = tr_swz(rrow);
  int g_off[4], x_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    g_off[i] = tr_off(rrow, (wm * 64 + i * 16) >> 4, f, pp);
    x_off[i] = TILE_BYTES + tr_off(rrow, (wn * 64 + i * 16) >> 4, f, pp);
  }

  f32x4_t acc[4][4], acc1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc1[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  const bool do_colsum = (tk == 0) && (wn == 0) && (p.dbias != nullptr);
  bf16x8_t ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = f32_to_elem<F16>(1.0f);

  if (m_end > m_begin)
    tr_ring<F16>(smem, m_begin, ceil_div(m_end - m_begin, BK), stage_load, g_off, x_off, do_colsum, ones, acc, acc1);

  // ---- store: a lane holds packed columns kp .. kp + 3 of row o ----
  const int fr = lane & 15;
  const float beta = p.beta;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = o0 + wm * 64 + i * 16 + fr;
    if (o >= p.O) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kp = k0 + wn * 64 + j * 16 + grp4 * 4;
      if (kp >= p.K) continue;
      const f32x4_t a = acc[i][j];
      if (p.slab) {
        *(f32x4_t*)(p.slab + ((int64_t)slice * p.O + o) * p.K + kp) = a;
      } else if (p.hw == 1) {
        f32x4_t* d = (f32x4_t*)(p.dw + (int64_t)o * p.K + kp);
        f32x4_t v = a;
        if (beta != 0.f) v += *d * beta;
        *d = v;
      } else {   // C is a multiple of 8: the four packed columns are channels c .. c + 3 of one position
        const int pos = kp / p.C, c = kp - pos * p.C;
        float* d = p.dw + (int64_t)o * p.K + (int64_t)c * p.hw + pos;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = a[e];
          if (beta != 0.f) v += d[e * p.hw] * beta;
          d[e * p.hw] = v;
        }
      }
    }
    if (do_colsum && grp4 == 0) {
      if (p.slab) {
        p.colsum[(int64_t)slice * p.O + o] = acc1[i][0];
      } else {
        float v = acc1[i][0];
        if (beta != 0.f) v += p.dbias[o] * beta;
        p.dbias[o] = v;
      }
    }
  }
}

__global__ __launch_bounds__(NT) void linear_wgrad_finalize_kernel(const WgradArgs p, int slices) {
  const int64_t total = (int64_t)p.O * p.K;
  const int64_t step = total;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    const int64_t o = idx / p.K;
    const int j = (int)(idx - o * p.K);
    const int kp = p.hw == 1 ? j : (j % p.hw) * p.C + j / p.hw;
    const float* s = p.slab + o * p.K + kp;
    float v = s[0];
    for (int k = 1; k < slices; ++k) v += s[k * step];
    if (p.beta != 0.f) v += p.dw[idx] * p.beta;
    p.dw[idx] = v;
    if (idx < p.O && p.dbias) {
      float b = p.colsum[idx];
      for (int k = 1; k < slices; ++k) b += p.colsum[(int64_t)k * p.O + idx];
      if (p.beta != 0.f) b += p.dbias[idx] * p.beta;
      p.dbias[idx] = b;
    }
  }
}

// ---- weight pack ------------------------------------------------------------------------------------------------------
// w_fwd[o][kp] and w_dgrad[kp][o] for o < Op, kp < K: the value of w[o][logical(kp)] rounded to the element type, zero in
// the pad rows.  One thread per element of each copy, walking that copy in storage order.
template <bool F16>
__global__ __launch_bounds__(NT) void linear_pack_kernel(const float* __restrict__ w, int64_t s_o, int64_t s_k, int O,
                                                         int Op, int K, int C, int hw, bf16_t* __restrict__ w_fwd,
                                                         bf16_t* __restrict__ w_dgrad) {
  const int64_t total = (int64_t)Op * K;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    if (w_fwd) {
      const int64_t o = idx / K;
      const int kp = (int)(idx - o * K);
      const int j = hw == 1 ? kp : (kp % C) * hw + kp / C;
      w_fwd[idx] = f32_to_elem<F16>(o < O ? w[o * s_o + j * s_k] : 0.f);
    }
    if (w_dgrad) {
      const int64_t kp = idx / Op;
      const int o = (int)(idx - kp * Op);
      const int64_t j = hw == 1 ? kp : (kp % C) * hw + kp / C;
      w_dgrad[idx] = f32_to_elem<F16>(o < O ? w[o * s_o + j * s_k] : 0.f);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct LinPlan {
  int rows, cols;          // extent of the product's output (wgrad: O x K)
  int tiles_r, tiles_c, tiles, chunks, slices, cps, launches, pad;
  int conv;                // the unsplit forward / dgrad of a layer with O % 64 == 0 goes to the conv GEMM (see below)
  int64_t slab_bytes;
};

int check_shape(const char* who, int kind, int M, int O, int K, int splits) {
  TDN_CHECK(kind >= 0 && kind <= 2, "%s: kind %d is none of 0 (forward), 1 (dgrad), 2 (wgrad)", who, kind);
  TDN_CHECK(M >= 0 && M <= MAX_M, "%s: M=%d out of 0..%d", who, M, MAX_M);
  TDN_CHECK(O >= 1 && O <= MAX_O, "%s: O=%d out of 1..%d", who, O, MAX_O);
  TDN_CHECK(K >= 64 && K <= MAX_K && K % 64 == 0, "%s: K=%d must be a multiple of 64 in 64..%d (K %% 64 != 0?)", who, K, MAX_K);
  const int hi = kind == 2 ? (M + 63) / 64 : K / 64;
  TDN_CHECK(splits >= 0 && (splits == 0 || splits <= (hi < 1 ? 1 : hi)), "%s: splits=%d out of range 0..%d", who, splits,
            hi < 1 ? 1 : hi);
  return 0;
}

// The split rule.  A product whose tiles already give every CU a workgroup is not cut; otherwise the slice count aims at
// FILL_WGS workgroups with a minimum of chunks per slice: 4 for a weight gradient and for ragged O.  Where the unsplit
// product can go to the conv GEMM instead (forward / dgrad, O % 64 == 0) the measurements are stricter: cut only below
// FILL_WGS / 2 tiles and never under 16 chunks per slice — fc6's forward at B = 2 (64 tiles, 196 chunks) is cut in 4 and
// beats the conv GEMM, at B = 4 (128 tiles) and for fc7 (16 chunks) the conv GEMM is faster and gets the product.
void make_plan(int kind, int M, int O, int K, int splits, LinPlan& pl) {
  const int Op = round64(O);
  if (kind == 0) { pl.rows = M; pl.cols = O; pl.chunks = K / BK; }
  else if (kind == 1) { pl.rows = M; pl.cols = K; pl.chunks = Op / BK; }
  else { pl.rows = O; pl.cols = K; pl.chunks = (M + BK - 1) / BK; }
  pl.tiles_r = (pl.rows + BM - 1) / BM;
  pl.tiles_c = (pl.cols + BN - 1) / BN;
  pl.tiles = pl.tiles_r * pl.tiles_c;
  const bool strict = kind != 2 && O % 64 == 0;
  const Split sp = split_rule(pl.tiles, pl.chunks, splits, strict ? FILL_WGS / 2 : FILL_WGS, strict ? 16 : 4);
  pl.cps = sp.cps;
  pl.slices = sp.slices > 0 ? sp.slices : 1;              // an empty product still counts as one slice
  pl.pad = (kind != 0 && (O % 64) != 0 && M > 0) ? 1 : 0;
  pl.conv = (splits == 0 && kind != 2 && O % 64 == 0 && pl.slices == 1 && M > 0) ? 1 : 0;
  const bool empty = kind != 2 && M == 0;
  pl.launches = empty ? 0 : pl.pad + 1 + (pl.slices > 1 ? 1 : 0);
  pl.slab_bytes = 0;
  if (pl.slices > 1) {
    const int64_t ld = kind == 2 ? K : round64(pl.cols);
    pl.slab_bytes = (int64_t)pl.slices * pl.rows * ld * 4;
  }
}

struct LinWs { bf16_t* gpad; float* slab; float* colsum; int64_t bytes; };
LinWs ws_layout(int kind, int M, int O, int K, const LinPlan& pl, void* base) {
  tdn_carver c{(char*)base, 0};
  LinWs w{nullptr, nullptr, nullptr, 0};
  if (pl.pad) w.gpad = c.take<bf16_t>((int64_t)M * round64(O));
  if (pl.slices > 1) {
    w.slab = c.take<float>(pl.slab_bytes / 4);
    if (kind == 2) w.colsum = c.take<float>((int64_t)pl.slices * O);
  }
  w.bytes = c.off;
  return w;
}

int check_ws(const char* who, const void* workspace, int64_t workspace_bytes, int64_t need) {
  if (need == 0) return 0;
  return tdn_check_ws(who, workspace, workspace_bytes, need);
}

template <bool F16>
int launch_gemm(const char* who, GemmArgs& p, const LinPlan& pl, hipStream_t stream) {
  if (tdn_allow_lds<linear_gemm_kernel<F16>>(LDS_BYTES, "linear_gemm_kernel") < 0) return -1;
  TDN_LAUNCH(linear_gemm_kernel<F16>, dim3((unsigned)(pl.tiles * pl.slices)), dim3(NT), LDS_BYTES, stream, p);
  TDN_LAUNCH_CHECK();
  if (pl.slices > 1) {
    const int grid = tdn_grid_1d((int64_t)p.M * p.N, NT, 4096);
    const int slices = pl.slices;
    TDN_LAUNCH(linear_finalize_kernel<F16>, dim3(grid), dim3(NT), 0, stream, p, slices);
    TDN_LAUNCH_CHECK();
  }
  (void)who;
  return 0;
}

int launch_pad(const void* g, int64_t ldg, bf16_t* gp, int M, int O, hipStream_t stream) {
  const int Op = round64(O);
  const int grid = tdn_grid_1d((int64_t)M * Op, NT, 4096);
  TDN_LAUNCH(linear_pad_kernel, dim3(grid), dim3(NT), 0, stream, (const bf16_t*)g, ldg, gp, M, O, Op);
  TDN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int tdn_pack_linear_weight(const float* w, int64_t s_o, int64_t s_k, int O, int K, int C, void* w_fwd,
                                      void* w_dgrad, int dtype, void* stream) {
  const char* who = "tdn_pack_linear_weight";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 0, 0, O, K, 0) != 0) return -1;
  TDN_CHECK(w && w_fwd, "%s: NULL pointer", who);
  TDN_CHECK(C >= 1 && C <= K && K % C == 0 && (C == K || C % 8 == 0), "%s: C=%d must divide K=%d and be a multiple of 8",
            who, C, K);
  TDN_CHECK(aligned(w_fwd, 16) && aligned(w_dgrad, 16), "%s: packed weights must be 16-byte aligned", who);
  const int Op = round64(O), hw = K / C;
  const int grid = tdn_grid_1d((int64_t)Op * K, NT, 4096);
  TDN_LAUNCH_T(linear_pack_kernel, dtype, dim3(grid), dim3(NT), stream, w, s_o, s_k, O, Op, K, C, hw, (bf16_t*)w_fwd,
               (bf16_t*)w_dgrad);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_linear_relu_bwd(const void* g, const void* y, int y_f32, void* out, int M, int O, int dtype,
                                   void* stream) {
  const char* who = "tdn_linear_relu_bwd";
  TDN_CHECK_DTYPE(dtype);
  TDN_CHECK(M >= 0 && M <= MAX_M && O >= 1 && O <= MAX_O, "%s: M=%d, O=%d out of range", who, M, O);
  if (M == 0) return 0;
  TDN_CHECK(g && y && out, "%s: NULL pointer", who);
  const int64_t n = (int64_t)M * O;
  TDN_LAUNCH_T(linear_relu_bwd_kernel, dtype, dim3(tdn_grid_1d(n, NT, 4096)), dim3(NT), stream, (const bf16_t*)g, y,
               y_f32 ? 1 : 0, (bf16_t*)out, n);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_linear_workspace_bytes(int kind, int M, int O, int K, int splits) {
  if (check_shape("tdn_linear_workspace_bytes", kind, M, O, K, splits) != 0) return -1;
  LinPlan pl;
  make_plan(kind, M, O, K, splits, pl);
  return ws_layout(kind, M, O, K, pl, nullptr).bytes;
}

extern "C" int tdn_linear_plan(int kind, int M, int O, int K, int splits, int32_t* out) {
  const char* who = "tdn_linear_plan";
  if (check_shape(who, kind, M, O, K, splits) != 0) return -1;
  TDN_CHECK(out, "%s: NULL out", who);
  LinPlan pl;
  make_plan(kind, M, O, K, splits, pl);
  const int64_t ws = ws_layout(kind, M, O, K, pl, nullptr).bytes;
  write_plan(out, pl.tiles_r, pl.tiles_c, pl.slices, pl.cps, pl.chunks, pl.tiles * pl.slices, pl.launches,
             pl.pad + 2 * pl.conv, pl.slab_bytes, ws);
  return 0;
}

extern "C" int tdn_linear_fwd(const void* x, int64_t ldx, const void* w_fwd, const float* bias, void* y, int64_t ldy,
                              int M, int O, int K, int relu, int out_f32, int splits, void* workspace,
                              int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_linear_fwd";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 0, M, O, K, splits) != 0) return -1;
  if (M == 0) return 0;
  TDN_CHECK(x && w_fwd && y, "%s: NULL pointer", who);
  TDN_CHECK(ldx >= K && ldx % 8 == 0 && aligned(x, 16), "%s: x rows must be 16-byte aligned (ldx=%lld)", who, (long long)ldx);
  TDN_CHECK(aligned(w_fwd, 16), "%s: w_fwd must be 16-byte aligned", who);
  TDN_CHECK(ldy >= O, "%s: ldy=%lld < O=%d", who, (long long)ldy, O);
  LinPlan pl;
  make_plan(0, M, O, K, splits, pl);
  const LinWs w = ws_layout(0, M, O, K, pl, workspace);
  if (check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  if (pl.conv && ldx == K && ldy == O) {   // a 1x1 conv over M pixels: w_fwd [O][K] is the conv pack's [O][1][1][K]
    tdn_epilogue ep{};
    ep.shift = bias; ep.relu = relu ? 1 : 0; ep.out_f32 = out_f32 ? 1 : 0;
    return tdn_conv2d_fwd(x, w_fwd, y, 1, M, 1, K, O, 1, 1, 0, &ep, dtype, stream);
  }
  GemmArgs p{};
  p.A = (const bf16_t*)x; p.lda = ldx; p.a_rows = M;
  p.B = (const bf16_t*)w_fwd; p.ldb = K; p.b_rows = round64(O);
  p.M = M; p.N = O;
  p.nchunks = pl.chunks; p.cps = pl.cps; p.tiles_n = pl.tiles_c; p.ntiles = pl.tiles;
  p.out = y; p.ldo = ldy; p.out_f32 = out_f32 ? 1 : 0;
  p.bias = bias; p.relu = relu ? 1 : 0;
  p.mask = nullptr; p.ldmask = 0;
  p.vec = (ldy % 4 == 0) && aligned(y, 16) && (!bias || aligned(bias, 16));
  p.slab = w.slab; p.slab_ld = round64(O);
  return dtype == TDN_F16 ? launch_gemm<true>(who, p, pl, (hipStream_t)stream) : launch_gemm<false>(who, p, pl, (hipStream_t)stream);
}

extern "C" int tdn_linear_dgrad(const void* g, int64_t ldg, const void* w_dgrad, const void* mask_src, int64_t ld_mask,
                                void* dx, int64_t lddx, int M, int O, int K, int splits, void* workspace,
                                int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_linear_dgrad";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 1, M, O, K, splits) != 0) return -1;
  if (M == 0) return 0;
  TDN_CHECK(g && w_dgrad && dx, "%s: NULL pointer", who);
  TDN_CHECK(ldg >= O && lddx >= K && (!mask_src || ld_mask >= K), "%s: a leading dimension is shorter than its row", who);
  TDN_CHECK(aligned(w_dgrad, 16), "%s: w_dgrad must be 16-byte aligned", who);
  LinPlan pl;
  make_plan(1, M, O, K, splits, pl);
  const LinWs w = ws_layout(1, M, O, K, pl, workspace);
  if (check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  const int Op = round64(O);
  if (pl.conv && ldg == O && lddx == K && (!mask_src || ld_mask == K)) {   // w_dgrad [K][O] is the conv pack's [K][1][1][O]
    tdn_epilogue ep{};
    ep.mask_src = mask_src;
    return tdn_conv2d_dgrad(g, w_dgrad, dx, 1, M, 1, K, O, 1, 1, 0, &ep, dtype, stream);
  }
  if (pl.pad) {
    TDN_CHECK(aligned(g, 2), "%s: g must be 2-byte aligned", who);
    if (launch_pad(g, ldg, w.gpad, M, O, (hipStream_t)stream) != 0) return -2;
  } else {
    TDN_CHECK(ldg % 8 == 0 && aligned(g, 16), "%s: g rows must be 16-byte aligned when O is a multiple of 64 (ldg=%lld)",
              who, (long long)ldg);
  }
  GemmArgs p{};
  p.A = pl.pad ? w.gpad : (const bf16_t*)g; p.lda = pl.pad ? Op : ldg; p.a_rows = M;
  p.B = (const bf16_t*)w_dgrad; p.ldb = Op; p.b_rows = K;
  p.M = M; p.N = K;
  p.nchunks = pl.chunks; p.cps = pl.cps; p.tiles_n = pl.tiles_c; p.ntiles = pl.tiles;
  p.out = dx; p.ldo = lddx; p.out_f32 = 0;
  p.bias = nullptr; p.relu = 0;
  p.mask = (const bf16_t*)mask_src; p.ldmask = ld_mask;
  p.vec = (lddx % 4 == 0) && aligned(dx, 8) && (!mask_src || (ld_mask % 4 == 0 && aligned(mask_src, 8)));
  p.slab = w.slab; p.slab_ld = round64(K);
  return dtype == TDN_F16 ? launch_gemm<true>(who, p, pl, (hipStream_t)stream) : launch_gemm<false>(who, p, pl, (hipStream_t)stream);
}

extern "C" int tdn_linear_wgrad(const void* x, int64_t ldx, const void* g, int64_t ldg, float* dw, float* dbias, float beta,
                                int M, int O, int K, int C, int splits, void* workspace, int64_t workspace_bytes,
                                int dtype, void* stream) {
  const char* who = "tdn_linear_wgrad";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 2, M, O, K, splits) != 0) return -1;
  TDN_CHECK(dw && (M == 0 || (x && g)), "%s: NULL pointer", who);
  TDN_CHECK(C >= 1 && C <= K && K % C == 0 && (C == K || C % 8 == 0), "%s: C=%d must divide K=%d and be a multiple of 8",
            who, C, K);
  TDN_CHECK(beta == beta, "%s: beta is NaN", who);
  TDN_CHECK(aligned(dw, 16), "%s: dw must be 16-byte aligned", who);
  TDN_CHECK(M == 0 || (ldx >= K && ldx % 8 == 0 && aligned(x, 16)), "%s: x rows must be 16-byte aligned (ldx=%lld)", who,
            (long long)ldx);
  TDN_CHECK(M == 0 || ldg >= O, "%s: ldg=%lld < O=%d", who, (long long)ldg, O);
  LinPlan pl;
  make_plan(2, M, O, K, splits, pl);
  const LinWs w = ws_layout(2, M, O, K, pl, workspace);
  if (check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  const int Op = round64(O);
  if (pl.pad) {
    if (launch_pad(g, ldg, w.gpad, M, O, (hipStream_t)stream) != 0) return -2;
  } else {
    TDN_CHECK(M == 0 || (ldg % 8 == 0 && aligned(g, 16)),
              "%s: g rows must be 16-byte aligned when O is a multiple of 64 (ldg=%lld)", who, (long long)ldg);
  }
  WgradArgs p{};
  p.g = pl.pad ? w.gpad : (const bf16_t*)g; p.ldg = pl.pad ? Op : ldg; p.g_cols = Op;
  p.x = (const bf16_t*)x; p.ldx = ldx;
  p.M = M; p.O = O; p.K = K; p.C = C; p.hw = K / C;
  p.mchunks = pl.chunks; p.cps = pl.cps; p.tiles_o = pl.tiles_r; p.ntiles = pl.tiles;
  p.dw = dw; p.dbias = dbias; p.beta = beta;
  p.slab = w.slab; p.colsum = w.colsum;
  return launch_wgrad<linear_wgrad_kernel<true>, linear_wgrad_kernel<false>, linear_wgrad_finalize_kernel>(
      "linear_wgrad_kernel", dtype == TDN_F16, pl.tiles * pl.slices, p, pl.slices > 1 ? (int64_t)O * K : 0, pl.slices,
      (hipStream_t)stream);
}
