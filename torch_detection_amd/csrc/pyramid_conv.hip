// A 3x3, stride-1, pad-1 convolution whose weights are shared by the levels of a feature pyramid: the
// tower layers and the two predictors of a single-stage head (RetinaHead).  One launch per product covers a table of up
// to 8 levels; the output-channel count Cout is any integer in 1..1024, the rows of the Cout-channel maps are dense
// (2 * Cout bytes, for odd Cout only 2-byte aligned).
//
//   forward   y_l[p][o]  = [relu](sum_{t,c} x_l[p + t][c] * W[o][t][c] + bias[o])                    pyr_conv_kernel<.., false>
//   dgrad     dx_l[p][c] = mask(sum_{t,o} g_l[p + t][o] * W[o][flip t][c] [+ addend_l[p][c]])        pyr_conv_kernel<.., true>
//   wgrad     dW[o][t][c] = sum over all levels and pixels of g_l[p][o] * x_l[p + t][c], dbias[o] = sum of g_l[p][o]
//                                                                          pyr_wgrad_kernel + pyr_wgrad_finalize_kernel
//
// p + t is the pixel one tap away inside the same map; taps outside the map contribute zero and are never read.  Forward
// and dgrad are ONE tiled implicit GEMM: a workgroup owns 128 consecutive pixels of one level (the flat (image, row,
// column) index, so a tile may straddle rows and images) and 64 output columns, and walks the reduction in steps of one
// tap x 64 input channels.  The 64 x 64 weight piece of a step is staged in LDS (two buffers, one barrier per step, the
// next pieces' loads in flight during the MFMAs); the activations go from global memory straight into MFMA operand
// registers, two steps ahead.  For dgrad the "input channels" are the Cout columns of the cotangent, read where they lie:
// the reduction is padded to 64 with zero weight columns and zero operand registers, never with a padded copy.
//
// The workgroups are numbered over the concatenated 128-pixel tiles of the levels and look their (level, first pixel)
// up in a table that travels in the kernel arguments, as in dense_head.hip.  Pixel offsets are 64-bit.
#include "pyramid_core.h"

namespace {

constexpr int NT = 256;               // 4 waves
constexpr int PB = 2;                 // 16-pixel blocks per wave (4 measured 15-20 % slower at the workload pyramid)
constexpr int PT = LEVEL_TILE;        // pixels per workgroup (forward, dgrad); pixels per wgrad step
static_assert(PT == 64 * PB, "4 waves x PB 16-pixel blocks");
constexpr int CT = 64;                // output columns per workgroup; channels per wgrad tile
constexpr int KC = 64;                // reduction elements per step
constexpr int MAXL = TDN_PYR_MAX_LEVELS;
constexpr int TRB = CT * 2 + 32;      // LDS row bytes of wgrad's tiles: the pad spreads 4 rows over distinct banks
constexpr int WG_TARGET = 1024;       // wgrad: about this many workgroups (slices x tiles)
constexpr int MAX_SLICES = 64;
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;

struct PyrArgs {
  const bf16_t* in[MAXL];             // forward: x; dgrad: g; wgrad: x
  bf16_t* out[MAXL];                  // forward: y; dgrad: dx
  const bf16_t* g[MAXL];              // wgrad: the cotangent
  const bf16_t* mask[MAXL];
  const bf16_t* add[MAXL];
  int64_t rows[MAXL];                 // B * H * W
  int H[MAXL], W[MAXL];
  int first[MAXL + 1];                // first pixel tile (forward, dgrad) or first slice (wgrad) of a level
  int n;
  int Kin, KP;                        // reduction elements per tap, and padded to 64
  int N;                              // output columns
  int relu, ragged;                   // ragged: the rows of `in` / `g` are not all 16-byte aligned runs of 8
  const bf16_t* w;
  const float* bias;
  int Cin, Cout, Cp;                  // wgrad
  int slice_rows, units, ctiles;
  float* slab;                        // [slice][Cp][9][Cin]
  float* colsum;                      // [slice][Cp]
};

// 8 elements k0 .. k0 + 7 of a Kin-element row; what lies at or beyond Kin reads as zero and is not touched
__device__ __forceinline__ bf16x8_t load_run(const bf16_t* row, int k0, int Kin, bool ragged) {
  if (!ragged) return k0 < Kin ? *(const bf16x8_t*)(row + k0) : zero8();
  const unsigned short* s = (const unsigned short*)row;
  s16x8_t v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = k0 + e < Kin ? (short)s[k0 + e] : (short)0;
  return __builtin_bit_cast(bf16x8_t, v);
}

// the 16-byte piece of a 128-byte LDS weight row is XOR-swizzled with the row bits that differ between the lanes of a read
__device__ __forceinline__ int w_swz(int row) { return ((row >> 1) & 1) | (((row >> 4) & 3) << 1); }

// ---- forward / dgrad ------------------------------------------------------------------------------------------------------
// packed weight [Np][9][KP]: column n, tap t, reduction element k.  A lane (r = lane & 15, q = lane >> 4) owns pixel r of
// each of its wave's two 16-pixel blocks and, of every 64-element step, the elements 16 q .. 16 q + 15 (two MFMAs).  Row
// i of weight block j stands for column (i >> 2) * 16 + j * 4 + (i & 3), so that after the four blocks a lane holds the 16
// consecutive columns 16 q .. 16 q + 15 of its pixel.
template <bool F16, bool DGRAD, bool RAGGED>
__global__ __launch_bounds__(NT) void pyr_conv_kernel(const PyrArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * CT * KC * 2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = find_level(p.first, p.n, (int)blockIdx.x);
  const int n0 = (int)blockIdx.y * CT;
  const int64_t M = p.rows[l];
  const int H = p.H[l], W = p.W[l];
  const int Kin = p.Kin, KP = p.KP, N = p.N;
  const int64_t row0 = (int64_t)((int)blockIdx.x - p.first[l]) * PT + wave * (16 * PB);
  const int r = lane & 15, q = lane >> 4;
  const bf16_t* const in = p.in[l];

  int64_t m[PB];
  bool ok[PB];
  int ph[PB], pw[PB];
#pragma unroll
  for (int rb = 0; rb < PB; ++rb) {
    m[rb] = row0 + rb * 16 + r;
    ok[rb] = m[rb] < M;
    const int mi = ok[rb] ? (int)m[rb] : 0;
    const int t = mi / W;
    pw[rb] = mi - t * W;
    ph[rb] = t % H;
  }
  const int cpk = KP / KC, steps = 9 * cpk;

  // the weight piece of a step: 64 rows x 128 bytes, two 16-byte pieces per thread
  const int wrow = tid >> 3, wpc = tid & 7;
  auto load_w = [&](int st, bf16x8_t* wv) {
    const int t = st / cpk, ch = st - t * cpk;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = wrow + it * 32;
      wv[it] = *(const bf16x8_t*)(p.w + ((int64_t)(n0 + row) * 9 + t) * KP + ch * KC + wpc * 8);
    }
  };
  auto store_w = [&](int buf, const bf16x8_t* wv) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = wrow + it * 32;
      *(bf16x8_t*)(smem + buf * (CT * KC * 2) + row * (KC * 2) + ((wpc ^ w_swz(row)) << 4)) = wv[it];
    }
  };
  // Aligned rows: every load is issued unconditionally from an address inside the map (the pixel itself where the tap
  // leaves the map, the row's last run where the step lies in the zero padding of the reduction) and the operand is
  // zeroed by a select when it is used — a branch around a load would make the compiler drain every outstanding load
  // at the next wait.  `valid` holds one bit per (block, half step).
  auto load_a = [&](int st, bf16x8_t (*a)[2], unsigned& valid) {
    const int t = st / cpk, ch = st - t * cpk;
    const int dh = t / 3 - 1, dw = t - (t / 3) * 3 - 1;
    valid = 0;
#pragma unroll
    for (int rb = 0; rb < PB; ++rb) {
      const int hh = ph[rb] + dh, ww = pw[rb] + dw;
      const bool v = ok[rb] && hh >= 0 && hh < H && ww >= 0 && ww < W;
      if constexpr (RAGGED) {
        const bf16_t* const row = in + (m[rb] + (int64_t)dh * W + dw) * Kin;
#pragma unroll
        for (int s = 0; s < 2; ++s) a[rb][s] = v ? load_run(row, ch * KC + q * 16 + s * 8, Kin, true) : zero8();
        valid = ~0u;
      } else {
        const int64_t pix = v ? m[rb] + (int64_t)dh * W + dw : (ok[rb] ? m[rb] : 0);
        const bf16_t* const row = in + pix * Kin;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int k0 = ch * KC + q * 16 + s * 8;
          a[rb][s] = *(const bf16x8_t*)(row + (k0 < Kin ? k0 : Kin - 8));
          if (v && k0 < Kin) valid |= 1u << (rb * 2 + s);
        }
      }
    }
  };

  f32x4_t acc[PB][4];
#pragma unroll
  for (int rb = 0; rb < PB; ++rb)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[rb][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // the loads run two steps ahead of the MFMAs: step st stores the weight piece of st + 1 (loaded during st - 1) into
  // the other LDS buffer, issues the loads of st + 2 and computes st from registers loaded during st - 2.  The three
  // activation register sets rotate by NAME over a loop unrolled by three (the step count is a multiple of 9): a copy
  // from one set to the next would wait for the loads just issued.
  bf16x8_t wv[2], a0[PB][2], a1[PB][2], a2[PB][2];
  unsigned v0 = 0, v1 = 0, v2 = 0;
  load_w(0, wv);
  load_a(0, a0, v0);
  store_w(0, wv);
  load_w(1, wv);                                     // steps is a multiple of 9
  load_a(1, a1, v1);
  __syncthreads();
  const int lrow = (r >> 2) * 16 + (r & 3);
  auto step = [&](int st, bf16x8_t (&ac)[PB][2], unsigned vc, bf16x8_t (&al)[PB][2], unsigned& vl) {
    // No branch around the store or the loads (the last two steps store and load a piece nobody uses): with straight
    // code the compiler counts the outstanding loads exactly and waits for the oldest ones only.
    store_w((st + 1) & 1, wv);                       // the other buffer: every wave left it before the last barrier
    const int nx = st + 2 < steps ? st + 2 : steps - 1;
    load_w(nx, wv);
    load_a(nx, al, vl);
    const char* const wl = smem + (st & 1) * (CT * KC * 2);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8_t op[PB];
#pragma unroll
      for (int rb = 0; rb < PB; ++rb) op[rb] = (vc >> (rb * 2 + s)) & 1 ? ac[rb][s] : zero8();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = lrow + j * 4;
        const bf16x8_t wf = lds_read_b128(wl + row * (KC * 2) + (((q * 2 + s) ^ w_swz(row)) << 4));
        // D[row = weight row][col = pixel]
#pragma unroll
        for (int rb = 0; rb < PB; ++rb) acc[rb][j] = mfma16<F16>(wf, op[rb], acc[rb][j]);
      }
    }
    __syncthreads();
  };
#pragma unroll 1
  for (int st = 0; st < steps; st += 3) {
    step(st, a0, v0, a2, v2);
    step(st + 1, a1, v1, a0, v0);
    step(st + 2, a2, v2, a1, v1);
  }

  const int c0 = n0 + q * 16;
  const int nvalid = N - c0 < 16 ? (N - c0 < 0 ? 0 : N - c0) : 16;
  float bias[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) bias[e] = (!DGRAD && p.bias && e < nvalid) ? p.bias[c0 + e] : 0.f;
#pragma unroll
  for (int rb = 0; rb < PB; ++rb) {
    if (!ok[rb] || nvalid == 0) continue;
    float v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j * 4 + e] = acc[rb][j][e] + bias[j * 4 + e];
    const int64_t off = m[rb] * N + c0;
    if constexpr (DGRAD) {                         // N is a multiple of 64: whole, 16-byte aligned runs
      if (p.add[l]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bf16x8_t ad = *(const bf16x8_t*)(p.add[l] + off + u * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[u * 8 + e] += elem_to_f32<F16>(ad[e]);
        }
      }
      if (p.mask[l]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bf16x8_t mk = *(const bf16x8_t*)(p.mask[l] + off + u * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[u * 8 + e] = elem_to_f32<F16>(mk[e]) > 0.f ? v[u * 8 + e] : 0.f;
        }
      }
    } else if (p.relu) {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    bf16x8_t o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e >> 3][e & 7] = f32_to_elem<F16>(v[e]);
    bf16_t* const dst = p.out[l] + off;
    const unsigned al = (unsigned)(uintptr_t)dst;
    // only the stores the address allows: a row of an odd-Cout map is 2-byte aligned
    if (nvalid == 16 && (al & 15) == 0) {
      *(bf16x8_t*)dst = o[0];
      *(bf16x8_t*)(dst + 8) = o[1];
    } else if (nvalid == 16 && (al & 7) == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bf16x4_t h4;
#pragma unroll
        for (int e = 0; e < 4; ++e) h4[e] = o[u >> 1][(u & 1) * 4 + e];
        *(bf16x4_t*)(dst + u * 4) = h4;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < nvalid) dst[e] = o[e >> 3][e & 7];
    }
  }
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------
// One workgroup per (slice, 64-row tile of Cout, tap, 64-channel tile).  A slice is a run of at most slice_rows pixels of
// ONE level; the slice list is the levels' runs in level order.  Steps of 128 pixels: the tap-shifted x tile [128][64]
// (zero where the tap leaves the map) and the zero-padded cotangent tile [128][64] are written to LDS with plain stores
// (the next step's loads are in flight meanwhile) and read back transposed (ds_read_b64_tr_b16).  Wave w owns channels
// 16 w .. + 15 of the tile and all 64 output rows.
template <bool F16>
__global__ __launch_bounds__(NT) void pyr_wgrad_kernel(const PyrArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * PT * TRB];
  char* const sH = smem;
  char* const sG = smem + PT * TRB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sidx = (int)blockIdx.x / p.units, unit = (int)blockIdx.x - sidx * p.units;
  const int ot = unit / (9 * p.ctiles), rem = unit - ot * 9 * p.ctiles;
  const int tap = rem / p.ctiles, ct = rem - tap * p.ctiles;
  const int dh = tap / 3 - 1, dw = tap - (tap / 3) * 3 - 1;
  const int l = find_level(p.first, p.n, sidx);
  const int Cin = p.Cin, Cout = p.Cout, H = p.H[l], W = p.W[l];
  const bool ragged = p.ragged;
  const int64_t m_begin = (int64_t)(sidx - p.first[l]) * p.slice_rows;
  const int64_t m_end = min(p.rows[l], m_begin + p.slice_rows);
  const bf16_t* const xl = p.in[l] + ct * CT;
  const bf16_t* const gl = p.g[l];
  const int prow = tid >> 3, ppc = tid & 7;          // a thread's row (of 32) and 16-byte piece in each of 4 passes

  bf16x8_t hv[4], gv[4];
  auto load_tile = [&](int64_t mt) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t m = mt + it * 32 + prow;
      const bool in_slice = m < m_end;
      const int mi = in_slice ? (int)m : 0;
      const int t = mi / W;
      const int ww = mi - t * W + dw, hh = t % H + dh;
      const bool v = in_slice && hh >= 0 && hh < H && ww >= 0 && ww < W;
      hv[it] = v ? *(const bf16x8_t*)(xl + (m + (int64_t)dh * W + dw) * Cin + ppc * 8) : zero8();
      gv[it] = in_slice ? load_run(gl + m * Cout, ot * CT + ppc * 8, Cout, ragged) : zero8();
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 32 + prow;
      *(bf16x8_t*)(sH + row * TRB + ppc * 16) = hv[it];
      *(bf16x8_t*)(sG + row * TRB + ppc * 16) = gv[it];
    }
  };

  // transposing reads: lane group g4 takes rows 8 g4 .. + 7 of a 32-row step, as two 4-row halves
  const int g4 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  const int rrow = 8 * g4 + qq;
  const int x_off = rrow * TRB + wave * 32 + pp * 8;
  const int g_off = rrow * TRB + pp * 8;

  f32x4_t acc[4], acc1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    acc1[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  const bool do_colsum = ct == 0 && tap == 0 && wave == 0;
  const bf16x8_t ones = wg_ones<F16>();

  const int T = (int)((m_end - m_begin + PT - 1) / PT);
  // D[row = channel][col = o] += sum_m x[m + tap][c] * g[m][o]
  wg_slice<4, TRB, TRB>(sH, sG, m_begin, T, load_tile, store_tile, x_off, g_off,
                        [&](int i, const bf16x8_t& xf, const char* gp) {
                          wg_mma<F16, TRB>(xf, gp, do_colsum, ones, acc[i], acc1[i]);
                        });
  // a lane holds channels c .. c + 3 of output row o
  const int fr = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = ot * CT + 16 * i + fr;
    const int c = ct * CT + wave * 16 + g4 * 4;
    *(f32x4_t*)(p.slab + (((int64_t)sidx * p.Cp + o) * 9 + tap) * Cin + c) = acc[i];
    if (do_colsum && g4 == 0) p.colsum[(int64_t)sidx * p.Cp + o] = acc1[i][0];
  }
}

// dW and dbias = the slabs added in slice order; dW is written through the parameter's own strides
__global__ __launch_bounds__(NT) void pyr_wgrad_finalize_kernel(const PyrArgs p, int slices, float* dw, int64_t s_o,
                                                                int64_t s_c, int64_t s_h, int64_t s_w, float* dbias) {
  const int Cin = p.Cin, Cout = p.Cout;
  const int64_t total = (int64_t)Cout * 9 * Cin;
  const int64_t step = (int64_t)p.Cp * 9 * Cin;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    const int c = (int)(idx % Cin);
    const int ot = (int)(idx / Cin);
    const int t = ot % 9, o = ot / 9;
    const float* s = p.slab + idx;
    float v = 0.f;
#pragma unroll 4
    for (int k = 0; k < slices; ++k) v += s[k * step];
    dw[o * s_o + c * s_c + (t / 3) * s_h + (t % 3) * s_w] = v;
    if (idx < Cout) {
      float b = 0.f;
      for (int k = 0; k < slices; ++k) b += p.colsum[(int64_t)k * p.Cp + idx];
      dbias[idx] = b;
    }
  }
}

// ---- weight pack ----------------------------------------------------------------------------------------------------------
// w_fwd [Cp][9][Cin]: w_fwd[o][3 kh + kw][c] = w[o][c][kh][kw]; w_dgrad [Cin][9][Cp]: w_dgrad[c][3 th + tw][o] =
// w[o][c][2 - th][2 - tw]; each value rounded once, zero for o >= Cout
template <bool F16>
__global__ __launch_bounds__(NT) void pyr_pack_kernel(const float* __restrict__ w, int64_t s_o, int64_t s_c, int64_t s_h,
                                                      int64_t s_w, int Cout, int Cin, int Cp, bf16_t* __restrict__ w_fwd,
                                                      bf16_t* __restrict__ w_dgrad) {
  const int total = Cp * 9 * Cin;
  for (int idx = (int)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int)gridDim.x * NT) {
    {
      const int c = idx % Cin, ot = idx / Cin, t = ot % 9, o = ot / 9;
      w_fwd[idx] = f32_to_elem<F16>(o < Cout ? w[o * s_o + c * s_c + (t / 3) * s_h + (t % 3) * s_w] : 0.f);
    }
    if (w_dgrad) {
      const int o = idx % Cp, ct = idx / Cp, t = ct % 9, c = ct / 9;
      w_dgrad[idx] = f32_to_elem<F16>(o < Cout ? w[o * s_o + c * s_c + (2 - t / 3) * s_h + (2 - t % 3) * s_w] : 0.f);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct PyrPlan {
  int Cp;
  LevelCut cut;            // forward / dgrad pixel tiles, wgrad slices
  int coltiles;            // forward / dgrad grid: cut.tiles x coltiles
  int units, ctiles;
  int lds;
  int first[MAXL + 1];
  int64_t rows[MAXL];
  int64_t slab_bytes;
};

int check_shape(const char* who, int kind, int B, const int32_t* hw, int n, int Cin, int Cout) {
  TDN_CHECK(kind >= 0 && kind <= 2, "%s: kind %d is none of 0 (forward), 1 (dgrad), 2 (wgrad)", who, kind);
  if (check_levels(who, n, MAXL) != 0) return -1;
  TDN_CHECK(hw, "%s: NULL level sizes", who);
  TDN_CHECK(B >= 0, "%s: B=%d is negative", who, B);
  TDN_CHECK(Cin >= 64 && Cin <= 512 && Cin % 64 == 0, "%s: Cin=%d must be a multiple of 64 in 64..512", who, Cin);
  TDN_CHECK(Cout >= 1 && Cout <= 1024, "%s: Cout=%d out of 1..1024", who, Cout);
  int64_t tiles = 0;
  for (int l = 0; l < n; ++l) {
    const int64_t H = hw[2 * l], W = hw[2 * l + 1];
    TDN_CHECK(H >= 1 && W >= 1 && H < MAX_ROWS && W < MAX_ROWS, "%s: level %d: H=%lld, W=%lld must be positive", who, l,
              (long long)H, (long long)W);
    TDN_CHECK(H * W < MAX_ROWS && (int64_t)B * H * W < MAX_ROWS, "%s: level %d: B*H*W out of 0..2^31-1", who, l);
    tiles += ((int64_t)B * H * W + PT - 1) / PT;
  }
  return check_tiles(who, tiles, "pixel");
}

void make_plan(int kind, int B, const int32_t* hw, int n, int Cin, int Cout, PyrPlan& pl) {
  pl.Cp = (Cout + CT - 1) / CT * CT;
  pl.ctiles = Cin / CT;
  pl.coltiles = kind == 1 ? pl.ctiles : pl.Cp / CT;
  pl.units = (pl.Cp / CT) * 9 * pl.ctiles;
  for (int l = 0; l < n; ++l) pl.rows[l] = (int64_t)B * hw[2 * l] * hw[2 * l + 1];
  // as many slices as bring the grid to about WG_TARGET workgroups, at most MAX_SLICES
  int target = (WG_TARGET + pl.units - 1) / pl.units;
  if (target > MAX_SLICES) target = MAX_SLICES;
  pl.cut = cut_levels(kind == 2, pl.rows, n, target, pl.first, MAXL);
  pl.lds = kind == 2 ? 2 * PT * TRB : 2 * CT * KC * 2;
  pl.slab_bytes = kind == 2 ? (int64_t)pl.cut.slices * pl.Cp * 9 * Cin * 4 : 0;
}

SlabWs ws_layout(int kind, const PyrPlan& pl, void* base) {
  return slab_layout(kind == 2 ? pl.cut.slices : 0, pl.slab_bytes, pl.Cp, base);
}

int sizes_of(const char* who, const tdn_pyr_level* levels, int n, int32_t* hw) {
  TDN_CHECK(levels, "%s: NULL levels", who);
  if (check_levels(who, n, MAXL) != 0) return -1;
  for (int l = 0; l < n; ++l) {
    hw[2 * l] = levels[l].H;
    hw[2 * l + 1] = levels[l].W;
  }
  return 0;
}

// kind 0: in = x (Cin), out = y (Cout); 1: in = y as the cotangent (Cout), out = dx (Cin); 2: in = x, g = y
int fill_args(const char* who, int kind, const tdn_pyr_level* levels, int n, int Cin, int Cout, const PyrPlan& pl,
              PyrArgs& p) {
  p = PyrArgs{};
  bool ragged = Cout % 8 != 0;
  for (int l = 0; l < n; ++l) {
    const tdn_pyr_level& L = levels[l];
    if (pl.rows[l] > 0) {
      TDN_CHECK(L.x || kind == 1, "%s: level %d: NULL x", who, l);
      TDN_CHECK(L.y, "%s: level %d: NULL %s", who, l, kind == 0 ? "y" : "cotangent");
      TDN_CHECK(kind != 1 || L.dx, "%s: level %d: NULL dx", who, l);
      TDN_CHECK(kind == 1 || aligned(L.x, 16), "%s: level %d: x must be 16-byte aligned", who, l);
      TDN_CHECK(aligned(L.y, 2), "%s: level %d: the Cout-channel map must be 2-byte aligned", who, l);
      if (kind == 1)
        TDN_CHECK(aligned(L.dx, 16) && aligned(L.mask_src, 16) && aligned(L.addend, 16),
                  "%s: level %d: dx, mask_src and addend must be 16-byte aligned", who, l);
      if (!aligned(L.y, 16)) ragged = true;
    }
    p.rows[l] = pl.rows[l];
    p.H[l] = L.H;
    p.W[l] = L.W;
    if (kind == 0) {
      p.in[l] = (const bf16_t*)L.x; p.out[l] = (bf16_t*)L.y;
    } else if (kind == 1) {
      p.in[l] = (const bf16_t*)L.y; p.out[l] = (bf16_t*)L.dx;
      p.mask[l] = (const bf16_t*)L.mask_src; p.add[l] = (const bf16_t*)L.addend;
    } else {
      p.in[l] = (const bf16_t*)L.x; p.g[l] = (const bf16_t*)L.y;
    }
  }
  for (int l = 0; l <= MAXL; ++l) p.first[l] = pl.first[l];
  p.n = n;
  p.Kin = kind == 1 ? Cout : Cin;
  p.KP = kind == 1 ? pl.Cp : Cin;
  p.N = kind == 1 ? Cin : Cout;
  p.ragged = ragged ? 1 : 0;
  p.Cin = Cin; p.Cout = Cout; p.Cp = pl.Cp;
  p.slice_rows = pl.cut.slice_rows; p.units = pl.units; p.ctiles = pl.ctiles;
  return 0;
}

}  // namespace

extern "C" int tdn_pack_pyr_weight(const float* w, int64_t s_o, int64_t s_c, int64_t s_h, int64_t s_w, int Cout, int Cin,
                                   void* w_fwd, void* w_dgrad, int dtype, void* stream) {
  const char* who = "tdn_pack_pyr_weight";
  TDN_CHECK_DTYPE(dtype);
  const int32_t one[2] = {1, 1};
  if (check_shape(who, 0, 0, one, 1, Cin, Cout) != 0) return -1;
  TDN_CHECK(w && w_fwd, "%s: NULL pointer", who);
  TDN_CHECK(aligned(w_fwd, 16) && aligned(w_dgrad, 16), "%s: packed weights must be 16-byte aligned", who);
  const int Cp = (Cout + CT - 1) / CT * CT;
  const int total = Cp * 9 * Cin;
  TDN_LAUNCH_T(pyr_pack_kernel, dtype, dim3(tdn_grid_1d(total, NT, 4096)), dim3(NT), stream, w, s_o, s_c, s_h, s_w, Cout,
               Cin, Cp, (bf16_t*)w_fwd, (bf16_t*)w_dgrad);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_pyr_workspace_bytes(int kind, int B, const int32_t* hw, int num_levels, int Cin, int Cout) {
  if (check_shape("tdn_pyr_workspace_bytes", kind, B, hw, num_levels, Cin, Cout) != 0) return -1;
  PyrPlan pl;
  make_plan(kind, B, hw, num_levels, Cin, Cout, pl);
  return ws_layout(kind, pl, nullptr).bytes;
}

extern "C" int tdn_pyr_plan(int kind, int B, const int32_t* hw, int num_levels, int Cin, int Cout, int32_t* out) {
  const char* who = "tdn_pyr_plan";
  if (check_shape(who, kind, B, hw, num_levels, Cin, Cout) != 0) return -1;
  TDN_CHECK(out, "%s: NULL out", who);
  PyrPlan pl;
  make_plan(kind, B, hw, num_levels, Cin, Cout, pl);
  const int64_t ws = ws_layout(kind, pl, nullptr).bytes;
  out[0] = PT;
  out[1] = kind == 2 ? pl.cut.slices * pl.units : pl.cut.tiles * pl.coltiles;
  out[2] = kind == 2 ? pl.cut.slices : 0;
  out[3] = kind == 2 ? pl.cut.slice_rows : 0;
  out[4] = pl.cut.launches;
  out[5] = CT;
  out[6] = pl.Cp;
  out[7] = kind == 1 ? pl.Cp : Cin;
  out[8] = pl.lds;
  out[9] = kind == 2 ? pl.units : pl.coltiles;
  out[10] = pl.cut.tiles;
  out[11] = 0;
  put_sizes(out, pl.slab_bytes, ws);
  return 0;
}

#define PYR_CONV(DG)                                                                                     \
  do {                                                                                                   \
    const dim3 grid((unsigned)pl.cut.tiles, (unsigned)pl.coltiles);                                          \
    if (DG && p.ragged) {                                                                                \
      if (dtype == TDN_F16) TDN_LAUNCH((pyr_conv_kernel<true, DG, DG>), grid, dim3(NT), 0, stream, p);   \
      else TDN_LAUNCH((pyr_conv_kernel<false, DG, DG>), grid, dim3(NT), 0, stream, p);                   \
    } else {                                                                                             \
      if (dtype == TDN_F16) TDN_LAUNCH((pyr_conv_kernel<true, DG, false>), grid, dim3(NT), 0, stream, p);  \
      else TDN_LAUNCH((pyr_conv_kernel<false, DG, false>), grid, dim3(NT), 0, stream, p);                \
    }                                                                                                    \
  } while (0)

extern "C" int tdn_pyr_conv_fwd(const tdn_pyr_level* levels, int num_levels, int B, const void* w_fwd, const float* bias,
                                int Cin, int Cout, int relu, int dtype, void* stream) {
  const char* who = "tdn_pyr_conv_fwd";
  TDN_CHECK_DTYPE(dtype);
  int32_t hw[2 * MAXL];
  if (sizes_of(who, levels, num_levels, hw) != 0 || check_shape(who, 0, B, hw, num_levels, Cin, Cout) != 0) return -1;
  PyrPlan pl;
  make_plan(0, B, hw, num_levels, Cin, Cout, pl);
  if (pl.cut.tiles == 0) return 0;
  TDN_CHECK(w_fwd && aligned(w_fwd, 16) && aligned(bias, 4), "%s: w_fwd must be a 16-byte aligned pointer", who);
  PyrArgs p;
  if (fill_args(who, 0, levels, num_levels, Cin, Cout, pl, p) != 0) return -1;
  p.w = (const bf16_t*)w_fwd; p.bias = bias; p.relu = relu ? 1 : 0;
  PYR_CONV(false);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_pyr_conv_dgrad(const tdn_pyr_level* levels, int num_levels, int B, const void* w_dgrad, int Cin,
                                  int Cout, int dtype, void* stream) {
  const char* who = "tdn_pyr_conv_dgrad";
  TDN_CHECK_DTYPE(dtype);
  int32_t hw[2 * MAXL];
  if (sizes_of(who, levels, num_levels, hw) != 0 || check_shape(who, 1, B, hw, num_levels, Cin, Cout) != 0) return -1;
  PyrPlan pl;
  make_plan(1, B, hw, num_levels, Cin, Cout, pl);
  if (pl.cut.tiles == 0) return 0;
  TDN_CHECK(w_dgrad && aligned(w_dgrad, 16), "%s: w_dgrad must be a 16-byte aligned pointer", who);
  PyrArgs p;
  if (fill_args(who, 1, levels, num_levels, Cin, Cout, pl, p) != 0) return -1;
  p.w = (const bf16_t*)w_dgrad;
  PYR_CONV(true);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_pyr_conv_wgrad(const tdn_pyr_level* levels, int num_levels, int B, float* dw, int64_t s_o, int64_t s_c,
                                  int64_t s_h, int64_t s_w, float* dbias, int Cin, int Cout, void* workspace,
                                  int64_t workspace_bytes, int dtype, void* stream) {
  const char* who = "tdn_pyr_conv_wgrad";
  TDN_CHECK_DTYPE(dtype);
  int32_t hw[2 * MAXL];
  if (sizes_of(who, levels, num_levels, hw) != 0 || check_shape(who, 2, B, hw, num_levels, Cin, Cout) != 0) return -1;
  TDN_CHECK(dw && dbias, "%s: NULL pointer", who);
  PyrPlan pl;
  make_plan(2, B, hw, num_levels, Cin, Cout, pl);
  const SlabWs w = ws_layout(2, pl, workspace);
  if (w.bytes && tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  PyrArgs p;
  if (fill_args(who, 2, levels, num_levels, Cin, Cout, pl, p) != 0) return -1;
  p.slab = w.slab; p.colsum = w.colsum;
  if (pl.cut.slices > 0) {
    const dim3 grid((unsigned)(pl.cut.slices * pl.units));
    if (dtype == TDN_F16) TDN_LAUNCH((pyr_wgrad_kernel<true>), grid, dim3(NT), 0, stream, p);
    else TDN_LAUNCH((pyr_wgrad_kernel<false>), grid, dim3(NT), 0, stream, p);
    TDN_LAUNCH_CHECK();
  }
  const int slices = pl.cut.slices;
  TDN_LAUNCH(pyr_wgrad_finalize_kernel, dim3(tdn_grid_1d((int64_t)Cout * 9 * Cin, NT, 4096)), dim3(NT), 0, stream, p, slices,
             dw, s_o, s_c, s_h, s_w, dbias);
  TDN_LAUNCH_CHECK();
  return 0;
}
