// The RPN head's two 1x1 predictors over a whole feature pyramid: a skinny shared-weight product over a
// table of up to 8 levels.  O = 5A output columns (A objectness rows, then 4A box rows; A <= 12), C input channels.
//
//   forward   cls_l[m][a] = h_l[m] . Wc[a] + bc[a],  reg_l[m][j] = h_l[m] . Wr[j] + br[j]      pred_fwd_kernel
//   dgrad     dh_l[m][c]  = h_l[m][c] > 0 ? sum_o g_l[m][o] * W[o][c] : 0                      pred_dgrad_kernel
//   wgrad     dW[o][c]    = sum over all levels and rows of g_l[m][o] * h_l[m][c], dbias[o] = sum of g_l[m][o]
//                                                                       pred_wgrad_kernel + pred_wgrad_finalize_kernel
//
// h_l is the hidden map of level l seen as an (M_l, C) matrix (NHWC memory); cls_l / reg_l and their cotangents are
// dense (M_l, A) and (M_l, 4A) matrices of their own.  Every product is a pure stream (per row 2C bytes in, 10A bytes
// out), so none of them stages the activations through an LDS ring: the packed weight (at most 64 KB) is staged ONCE per
// workgroup into LDS, the rows are read from global memory straight into MFMA operand registers.  The k index of an
// MFMA is a free permutation as long as both operands use the same one, and so is the column a lane of the weight
// operand stands for; both are chosen so that a lane reads and writes runs of 32 contiguous bytes of a row.
//
// One launch covers all levels: the workgroups are numbered over the concatenated 128-row tiles of the levels and look
// their (level, first row) up in a table that travels in the kernel arguments.  Row offsets are 64-bit.
#include "pyramid_core.h"

namespace {

constexpr int NT = 256;               // 4 waves
constexpr int RT = LEVEL_TILE;        // rows per workgroup (forward, dgrad): 2 x 16 rows per wave; rows per wgrad step
constexpr int MAXL = TDN_PRED_MAX_LEVELS;
constexpr int CT = 64;                // channels per wgrad workgroup
constexpr int HRB = CT * 2 + 32;      // LDS row bytes of wgrad's h tile: the pad spreads 4 rows over distinct banks
constexpr int SLICE_TARGET = 64;      // wgrad: the rows of all levels are cut into about this many slices
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;

struct PredArgs {
  const bf16_t* h[MAXL];
  bf16_t* cls[MAXL];
  bf16_t* reg[MAXL];
  bf16_t* dh[MAXL];
  int64_t rows[MAXL];
  int first[MAXL + 1];                // first workgroup (forward, dgrad) or first slice (wgrad) of a level
  int n, C, A, O;
  const bf16_t* w;                    // w_fwd [Op][C] or w_dgrad [C][Kp]
  const float* bc;
  const float* br;
  int slice_rows, ctiles;
  float* slab;                        // [slice][Op][C]
  float* colsum;                      // [slice][Op]
};

// ---- forward ------------------------------------------------------------------------------------------------------------
// LDS: w_fwd [16 NB][C], 16-byte piece pc of row r at position pc ^ (r & 7).  A lane (r = lane & 15, q = lane >> 4) owns
// row r of its 16-row block and, of every 128-byte chunk of that row, the 32 bytes q: two MFMA steps per chunk.
template <bool F16, int NB>
__global__ __launch_bounds__(NT) void pred_fwd_kernel(const PredArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = p.C, ppr = C >> 3;
  for (int idx = tid; idx < NB * 16 * ppr; idx += NT) {
    const int row = idx / ppr, pc = idx - row * ppr;
    *(bf16x8_t*)(smem + row * C * 2 + ((pc ^ (row & 7)) << 4)) = *(const bf16x8_t*)(p.w + (int64_t)row * C + pc * 8);
  }
  __syncthreads();
  const int l = find_level(p.first, p.n, (int)blockIdx.x);
  const int64_t M = p.rows[l];
  const int64_t row0 = (int64_t)((int)blockIdx.x - p.first[l]) * RT + wave * 32;
  const int r = lane & 15, q = lane >> 4;
  const int A = p.A, O = p.O;

  float bias[NB][4];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = 16 * j + 4 * q + e;
      bias[j][e] = n < A ? p.bc[n] : (n < O ? p.br[n - A] : 0.f);
    }

  const bf16_t* src[2];
  bool ok[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int64_t m = row0 + rb * 16 + r;
    ok[rb] = m < M;
    src[rb] = p.h[l] + m * C + q * 16;
  }
  f32x4_t acc[2][NB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[rb][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const char* wl = smem + r * C * 2;
  const int chunks = C >> 6;

  for (int t = 0; t < chunks; ++t) {
    bf16x8_t a[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int s = 0; s < 2; ++s) a[rb][s] = ok[rb] ? *(const bf16x8_t*)(src[rb] + t * 64 + s * 8) : zero8();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int piece = t * 8 + q * 2 + s;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const bf16x8_t wf = lds_read_b128(wl + j * 16 * C * 2 + ((piece ^ (r & 7)) << 4));
        // D[row = weight row][col = m]: a lane ends up with columns 16 j + 4 q .. + 3 of row r
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[rb][j] = mfma16<F16>(wf, a[rb][s], acc[rb][j]);
      }
    }
  }
  const int R4 = O - A;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    if (!ok[rb]) continue;
    const int64_t m = row0 + rb * 16 + r;
    bf16_t* const pc = p.cls[l] + m * A;
    bf16_t* const pr = p.reg[l] + m * R4;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = 16 * j + 4 * q + e;
        const bf16_t v = f32_to_elem<F16>(acc[rb][j][e] + bias[j][e]);
        if (n < A) pc[n] = v;
        else if (n < O) pr[n - A] = v;
      }
  }
}

// ---- dgrad ----------------------------------------------------------------------------------------------------------------
// LDS: w_dgrad [C][Kp], Kp = 32 KS; the 16-byte pieces of a row are XOR-swizzled with the channel bits that differ
// between the lanes of one read.  Lane (r, q) of weight block j stands for channel (j >> 2) * 64 + (r >> 2) * 16 +
// (j & 3) * 4 + (r & 3), so that after four blocks an output lane holds 16 consecutive channels of its row.
template <int KS>
__device__ __forceinline__ int dg_swz(int c) {
  if constexpr (KS == 1) return (c >> 4) & 3;
  else return ((c >> 1) & 1) | (((c >> 4) & 3) << 1);
}

template <bool F16, int KS>
__global__ __launch_bounds__(NT) void pred_dgrad_kernel(const PredArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KP = 32 * KS, PPR = 4 * KS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = p.C;
  for (int idx = tid; idx < C * PPR; idx += NT) {
    const int c = idx / PPR, pc = idx - c * PPR;
    *(bf16x8_t*)(smem + c * KP * 2 + ((pc ^ dg_swz<KS>(c)) << 4)) = *(const bf16x8_t*)(p.w + (int64_t)c * KP + pc * 8);
  }
  __syncthreads();
  const int l = find_level(p.first, p.n, (int)blockIdx.x);
  const int64_t M = p.rows[l];
  const int64_t row0 = (int64_t)((int)blockIdx.x - p.first[l]) * RT + wave * 32;
  const int r = lane & 15, q = lane >> 4;
  const int A = p.A, O = p.O, R4 = O - A;
  const unsigned short* const gc = (const unsigned short*)p.cls[l];
  const unsigned short* const gr = (const unsigned short*)p.reg[l];
  const int groups = C >> 6;
#pragma unroll 1
  for (int rb = 0; rb < 2; ++rb) {
    const int64_t m = row0 + rb * 16 + r;
    const bool ok = m < M;
    bf16x8_t a[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      s16x8_t v;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int o = s * 32 + q * 8 + t;
        unsigned short x = 0;
        if (ok) {
          if (o < A) x = gc[m * A + o];
          else if (o < O) x = gr[m * R4 + (o - A)];
        }
        v[t] = (short)x;
      }
      a[s] = __builtin_bit_cast(bf16x8_t, v);
    }
    const bf16_t* const hm = p.h[l] + m * C + q * 16;
    bf16_t* const out = p.dh[l] + m * C + q * 16;

    for (int jg = 0; jg < groups; ++jg) {
      bf16x8_t mk[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) mk[u] = ok ? *(const bf16x8_t*)(hm + jg * 64 + u * 8) : zero8();
      f32x4_t acc[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        acc[jj] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const int ch = jg * 64 + (r >> 2) * 16 + jj * 4 + (r & 3);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const bf16x8_t wf = lds_read_b128(smem + ch * KP * 2 + (((s * 4 + q) ^ dg_swz<KS>(ch)) << 4));
          acc[jj] = mfma16<F16>(wf, a[s], acc[jj]);
        }
      }
      if (ok) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          bf16x8_t o8;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = acc[u * 2 + (e >> 2)][e & 3];
            o8[e] = f32_to_elem<F16>(elem_to_f32<F16>(mk[u][e]) > 0.f ? v : 0.f);
          }
          *(bf16x8_t*)(out + jg * 64 + u * 8) = o8;
        }
      }
    }
  }
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------
// One workgroup per (slice, 64-channel tile).  A slice is a run of at most slice_rows rows of ONE level; the slice list is
// the levels' runs in level order.  Steps of 128 rows: the h tile [128][64] and the stacked, zero-padded cotangent tile
// [128][Op] are written to LDS with plain stores (the next step's loads are in flight meanwhile) and read back
// transposed (ds_read_b64_tr_b16).  Wave w owns channels 16 w .. + 15 of the tile and all Op output rows.
template <bool F16, int NB>
__global__ __launch_bounds__(NT) void pred_wgrad_kernel(const PredArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int OP = 16 * NB, GRB = OP * 2 + 32, GN = RT * OP / NT;
  char* const sH = smem;
  char* const sG = smem + RT * HRB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sidx = (int)blockIdx.x / p.ctiles, ct = (int)blockIdx.x - sidx * p.ctiles;
  const int l = find_level(p.first, p.n, sidx);
  const int C = p.C, A = p.A, O = p.O, R4 = O - A;
  const int64_t m_begin = (int64_t)(sidx - p.first[l]) * p.slice_rows;
  const int64_t m_end = min(p.rows[l], m_begin + p.slice_rows);
  const bf16_t* const hl = p.h[l] + ct * CT;
  const unsigned short* const gc = (const unsigned short*)p.cls[l];
  const unsigned short* const gr = (const unsigned short*)p.reg[l];

  bf16x8_t hv[4];
  unsigned short gv[GN];
  auto load_tile = [&](int64_t mt) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * NT + tid;
      const int64_t m = mt + (idx >> 3);
      hv[it] = m < m_end ? *(const bf16x8_t*)(hl + m * C + (idx & 7) * 8) : zero8();
    }
#pragma unroll
    for (int it = 0; it < GN; ++it) {
      const int idx = it * NT + tid;
      const int row = idx / OP, o = idx - row * OP;
      const int64_t m = mt + row;
      unsigned short x = 0;
      if (m < m_end) {
        if (o < A) x = gc[m * A + o];
        else if (o < O) x = gr[m * R4 + (o - A)];
      }
      gv[it] = x;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * NT + tid;
      *(bf16x8_t*)(sH + (idx >> 3) * HRB + (idx & 7) * 16) = hv[it];
    }
#pragma unroll
    for (int it = 0; it < GN; ++it) {
      const int idx = it * NT + tid;
      const int row = idx / OP, o = idx - row * OP;
      *(unsigned short*)(sG + row * GRB + o * 2) = gv[it];
    }
  };

  // transposing reads: lane group g4 takes rows 8 g4 .. + 7 of a 32-row step, as two 4-row halves
  const int g4 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  const int rrow = 8 * g4 + qq;
  const int x_off = rrow * HRB + wave * 32 + pp * 8;
  const int g_off = rrow * GRB + pp * 8;

  f32x4_t acc[NB], acc1[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    acc1[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  const bool do_colsum = ct == 0 && wave == 0;
  const bf16x8_t ones = wg_ones<F16>();

  // the text of pyramid_core.h's wg_slice, kept private: through it these kernels come out 13 to 62 VGPRs smaller, in
  // another schedule than the measured one, and <.., 3> spills two SGPRs (profiles/pyramid_core_refactor_checks.md)
  const int T = (int)((m_end - m_begin + RT - 1) / RT);
  if (T > 0) {
    load_tile(m_begin);
    store_tile();
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const bool more = t + 1 < T;
      if (more) load_tile(m_begin + (int64_t)(t + 1) * RT);
#pragma unroll
      for (int kk = 0; kk < RT / 32; ++kk) {
        const bf16x8_t xf = wg_frag<HRB>(sH + x_off + kk * 32 * HRB);
        // D[row = channel][col = o] += sum_m h[m][c] * g[m][o]
#pragma unroll
        for (int i = 0; i < NB; ++i)
          wg_mma<F16, GRB>(xf, sG + g_off + i * 32 + kk * 32 * GRB, do_colsum, ones, acc[i], acc1[i]);
      }
      __syncthreads();                      // every wave has read step t
      if (more) store_tile();
      __syncthreads();
    }
  }
  // a lane holds channels c .. c + 3 of output row o
  const int fr = lane & 15;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int o = 16 * i + fr;
    const int c = ct * CT + wave * 16 + g4 * 4;
    *(f32x4_t*)(p.slab + ((int64_t)sidx * OP + o) * C + c) = acc[i];
    if (do_colsum && g4 == 0) p.colsum[(int64_t)sidx * OP + o] = acc1[i][0];
  }
}

// dW and dbias = the slabs added in slice order, written in the two parameters' own (A, C) / (4A, C) layouts
__global__ __launch_bounds__(NT) void pred_wgrad_finalize_kernel(const PredArgs p, int slices, int Op, float* dwc, float* dbc,
                                                                 float* dwr, float* dbr) {
  const int C = p.C, A = p.A;
  const int total = p.O * C;
  const int64_t step = (int64_t)Op * C;
  for (int idx = (int)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int)gridDim.x * NT) {
    const int o = idx / C;
    const float* s = p.slab + idx;
    float v = 0.f;
#pragma unroll 8
    for (int k = 0; k < slices; ++k) v += s[k * step];
    if (o < A) dwc[idx] = v;
    else dwr[idx - A * C] = v;
    if (idx < p.O) {
      float b = 0.f;
      for (int k = 0; k < slices; ++k) b += p.colsum[(int64_t)k * Op + idx];
      if (idx < A) dbc[idx] = b;
      else dbr[idx - A] = b;
    }
  }
}

// ---- weight pack ----------------------------------------------------------------------------------------------------------
// w_fwd [Op][C] and w_dgrad [C][Kp]: the stacked weight (cls rows, then reg rows) rounded once, zero in the pad rows
template <bool F16>
__global__ __launch_bounds__(NT) void pred_pack_kernel(const float* __restrict__ wc, int64_t c_so, int64_t c_sc,
                                                       const float* __restrict__ wr, int64_t r_so, int64_t r_sc, int A,
                                                       int O, int Op, int Kp, int C, bf16_t* __restrict__ w_fwd,
                                                       bf16_t* __restrict__ w_dgrad) {
  const int total = (Op > Kp ? Op : Kp) * C;
  auto val = [&](int o, int c) {
    return o < A ? wc[o * c_so + c * c_sc] : (o < O ? wr[(o - A) * r_so + c * r_sc] : 0.f);
  };
  for (int idx = (int)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int)gridDim.x * NT) {
    if (idx < Op * C) w_fwd[idx] = f32_to_elem<F16>(val(idx / C, idx % C));
    if (w_dgrad && idx < Kp * C) w_dgrad[idx] = f32_to_elem<F16>(val(idx % Kp, idx / Kp));
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct PredPlan {
  int Op, Kp, NB, KS;
  LevelCut cut;            // forward / dgrad workgroups, wgrad slices
  int ctiles;
  int first[MAXL + 1];
  int64_t slab_bytes;
};

int check_shape(const char* who, int kind, const int64_t* rows, int n, int C, int A) {
  TDN_CHECK(kind >= 0 && kind <= 2, "%s: kind %d is none of 0 (forward), 1 (dgrad), 2 (wgrad)", who, kind);
  if (check_levels(who, n, MAXL) != 0) return -1;
  TDN_CHECK(rows, "%s: NULL rows", who);
  TDN_CHECK(C >= 64 && C <= 512 && C % 64 == 0, "%s: C=%d must be a multiple of 64 in 64..512", who, C);
  TDN_CHECK(A >= 1 && A <= 12, "%s: A=%d out of 1..12", who, A);
  int64_t tiles = 0;
  for (int l = 0; l < n; ++l) {
    TDN_CHECK(rows[l] >= 0 && rows[l] < MAX_ROWS, "%s: rows[%d]=%lld out of 0..2^31-1", who, l, (long long)rows[l]);
    tiles += (rows[l] + RT - 1) / RT;
  }
  return check_tiles(who, tiles, "row");
}

void make_plan(int kind, const int64_t* rows, int n, int C, int A, PredPlan& pl) {
  const int O = 5 * A;
  pl.Op = (O + 15) & ~15;
  pl.Kp = (O + 31) & ~31;
  pl.NB = pl.Op / 16;
  pl.KS = pl.Kp / 32;
  pl.ctiles = C / CT;
  pl.cut = cut_levels(kind == 2, rows, n, SLICE_TARGET, pl.first, MAXL);
  pl.slab_bytes = kind == 2 ? (int64_t)pl.cut.slices * pl.Op * C * 4 : 0;
}

SlabWs ws_layout(int kind, const PredPlan& pl, void* base) {
  return slab_layout(kind == 2 ? pl.cut.slices : 0, pl.slab_bytes, pl.Op, base);
}

int fill_args(const char* who, int kind, const tdn_pred_level* levels, int n, int C, int A, const PredPlan& pl, PredArgs& p) {
  p = PredArgs{};
  for (int l = 0; l < n; ++l) {
    const tdn_pred_level& L = levels[l];
    if (L.rows > 0) {
      TDN_CHECK(L.h && L.cls && L.reg && (kind != 1 || L.dh), "%s: NULL pointer in level %d", who, l);
      TDN_CHECK(aligned(L.h, 16) && (kind != 1 || aligned(L.dh, 16)), "%s: level %d: h and dh must be 16-byte aligned", who, l);
      TDN_CHECK(aligned(L.cls, 2) && aligned(L.reg, 2), "%s: level %d: cls and reg must be 2-byte aligned", who, l);
    }
    p.h[l] = (const bf16_t*)L.h; p.cls[l] = (bf16_t*)L.cls; p.reg[l] = (bf16_t*)L.reg; p.dh[l] = (bf16_t*)L.dh;
    p.rows[l] = L.rows;
  }
  for (int l = 0; l <= MAXL; ++l) p.first[l] = pl.first[l];
  p.n = n; p.C = C; p.A = A; p.O = 5 * A;
  p.slice_rows = pl.cut.slice_rows; p.ctiles = pl.ctiles;
  return 0;
}

int rows_of(const char* who, const tdn_pred_level* levels, int n, int64_t* rows) {
  TDN_CHECK(levels, "%s: NULL levels", who);
  if (check_levels(who, n, MAXL) != 0) return -1;
  for (int l = 0; l < n; ++l) rows[l] = levels[l].rows;
  return 0;
}

#define PRED_BY_NB(F16, nb, CALL)            \
  switch (nb) {                              \
    case 1: { CALL(F16, 1); } break;         \
    case 2: { CALL(F16, 2); } break;         \
    case 3: { CALL(F16, 3); } break;         \
    default: { CALL(F16, 4); } break;        \
  }

}  // namespace

extern "C" int tdn_pack_pred_weight(const float* w_cls, int64_t c_so, int64_t c_sc, const float* w_reg, int64_t r_so,
                                    int64_t r_sc, int A, int C, void* w_fwd, void* w_dgrad, int dtype, void* stream) {
  const char* who = "tdn_pack_pred_weight";
  TDN_CHECK_DTYPE(dtype);
  const int64_t none = 0;
  if (check_shape(who, 0, &none, 1, C, A) != 0) return -1;
  TDN_CHECK(w_cls && w_reg && w_fwd, "%s: NULL pointer", who);
  TDN_CHECK(aligned(w_fwd, 16) && aligned(w_dgrad, 16), "%s: packed weights must be 16-byte aligned", who);
  PredPlan pl;
  make_plan(0, &none, 1, C, A, pl);
  const int total = (pl.Op > pl.Kp ? pl.Op : pl.Kp) * C;
  TDN_LAUNCH_T(pred_pack_kernel, dtype, dim3(tdn_grid_1d(total, NT, 4096)), dim3(NT), stream, w_cls, c_so, c_sc, w_reg, r_so,
               r_sc, A, 5 * A, pl.Op, pl.Kp, C, (bf16_t*)w_fwd, (bf16_t*)w_dgrad);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_pred_workspace_bytes(int kind, const int64_t* rows, int num_levels, int C, int A) {
  if (check_shape("tdn_pred_workspace_bytes", kind, rows, num_levels, C, A) != 0) return -1;
  PredPlan pl;
  make_plan(kind, rows, num_levels, C, A, pl);
  return ws_layout(kind, pl, nullptr).bytes;
}

extern "C" int tdn_pred_plan(int kind, const int64_t* rows, int num_levels, int C, int A, int32_t* out) {
  const char* who = "tdn_pred_plan";
  if (check_shape(who, kind, rows, num_levels, C, A) != 0) return -1;
  TDN_CHECK(out, "%s: NULL out", who);
  PredPlan pl;
  make_plan(kind, rows, num_levels, C, A, pl);
  const int64_t ws = ws_layout(kind, pl, nullptr).bytes;
  out[0] = RT;
  out[1] = kind == 2 ? pl.cut.slices * pl.ctiles : pl.cut.tiles;
  out[2] = kind == 2 ? pl.cut.slices : 0;
  out[3] = kind == 2 ? pl.cut.slice_rows : 0;
  out[4] = pl.cut.launches;
  out[5] = pl.Op; out[6] = pl.Kp; out[7] = kind == 2 ? pl.ctiles : 1;
  out[8] = kind == 0 ? pl.Op * C * 2 : (kind == 1 ? C * pl.Kp * 2 : RT * HRB + RT * (pl.Op * 2 + 32));
  out[9] = out[10] = out[11] = 0;
  put_sizes(out, pl.slab_bytes, ws);
  return 0;
}

extern "C" int tdn_pred_fwd(const tdn_pred_level* levels, int num_levels, const void* w_fwd, const float* bias_cls,
                            const float* bias_reg, int C, int A, int dtype, void* stream) {
  const char* who = "tdn_pred_fwd";
  TDN_CHECK_DTYPE(dtype);
  int64_t rows[MAXL];
  if (rows_of(who, levels, num_levels, rows) != 0 || check_shape(who, 0, rows, num_levels, C, A) != 0) return -1;
  PredPlan pl;
  make_plan(0, rows, num_levels, C, A, pl);
  if (pl.cut.tiles == 0) return 0;
  TDN_CHECK(w_fwd && bias_cls && bias_reg, "%s: NULL pointer", who);
  TDN_CHECK(aligned(w_fwd, 16) && aligned(bias_cls, 4) && aligned(bias_reg, 4), "%s: w_fwd must be 16-byte aligned", who);
  PredArgs p;
  if (fill_args(who, 0, levels, num_levels, C, A, pl, p) != 0) return -1;
  p.w = (const bf16_t*)w_fwd; p.bc = bias_cls; p.br = bias_reg;
  const int lds = pl.Op * C * 2;
#define PRED_FWD(F16, NBV)                                                                                   \
  if (tdn_allow_lds<pred_fwd_kernel<F16, NBV>>(65536, "pred_fwd_kernel") < 0) return -1;                     \
  TDN_LAUNCH((pred_fwd_kernel<F16, NBV>), dim3((unsigned)pl.cut.tiles), dim3(NT), lds, stream, p)
  if (dtype == TDN_F16) { PRED_BY_NB(true, pl.NB, PRED_FWD) } else { PRED_BY_NB(false, pl.NB, PRED_FWD) }
#undef PRED_FWD
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_pred_dgrad(const tdn_pred_level* levels, int num_levels, const void* w_dgrad, int C, int A, int dtype,
                              void* stream) {
  const char* who = "tdn_pred_dgrad";
  TDN_CHECK_DTYPE(dtype);
  int64_t rows[MAXL];
  if (rows_of(who, levels, num_levels, rows) != 0 || check_shape(who, 1, rows, num_levels, C, A) != 0) return -1;
  PredPlan pl;
  make_plan(1, rows, num_levels, C, A, pl);
  if (pl.cut.tiles == 0) return 0;
  TDN_CHECK(w_dgrad && aligned(w_dgrad, 16), "%s: w_dgrad must be a 16-byte aligned pointer", who);
  PredArgs p;
  if (fill_args(who, 1, levels, num_levels, C, A, pl, p) != 0) return -1;
  p.w = (const bf16_t*)w_dgrad;
  const int lds = C * pl.Kp * 2;
#define PRED_DGRAD(F16, KSV)                                                                                 \
  if (tdn_allow_lds<pred_dgrad_kernel<F16, KSV>>(65536, "pred_dgrad_kernel") < 0) return -1;                 \
  TDN_LAUNCH((pred_dgrad_kernel<F16, KSV>), dim3((unsigned)pl.cut.tiles), dim3(NT), lds, stream, p)
  if (dtype == TDN_F16) {
    if (pl.KS == 1) { PRED_DGRAD(true, 1); } else { PRED_DGRAD(true, 2); }
  } else {
    if (pl.KS == 1) { PRED_DGRAD(false, 1); } else { PRED_DGRAD(false, 2); }
  }
#undef PRED_DGRAD
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int tdn_pred_wgrad(const tdn_pred_level* levels, int num_levels, float* dw_cls, float* dbias_cls, float* dw_reg,
                              float* dbias_reg, int C, int A, void* workspace, int64_t workspace_bytes, int dtype,
                              void* stream) {
  const char* who = "tdn_pred_wgrad";
  TDN_CHECK_DTYPE(dtype);
  int64_t rows[MAXL];
  if (rows_of(who, levels, num_levels, rows) != 0 || check_shape(who, 2, rows, num_levels, C, A) != 0) return -1;
  TDN_CHECK(dw_cls && dbias_cls && dw_reg && dbias_reg, "%s: NULL pointer", who);
  PredPlan pl;
  make_plan(2, rows, num_levels, C, A, pl);
  const SlabWs w = ws_layout(2, pl, workspace);
  if (w.bytes && tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  PredArgs p;
  if (fill_args(who, 2, levels, num_levels, C, A, pl, p) != 0) return -1;
  p.slab = w.slab; p.colsum = w.colsum;
  if (pl.cut.slices > 0) {
    const int lds = RT * HRB + RT * (pl.Op * 2 + 32);
    const dim3 grid((unsigned)(pl.cut.slices * pl.ctiles));
#define PRED_WGRAD(F16, NBV) TDN_LAUNCH((pred_wgrad_kernel<F16, NBV>), grid, dim3(NT), lds, stream, p)
    if (dtype == TDN_F16) { PRED_BY_NB(true, pl.NB, PRED_WGRAD) } else { PRED_BY_NB(false, pl.NB, PRED_WGRAD) }
#undef PRED_WGRAD
    TDN_LAUNCH_CHECK();
  }
  const int slices = pl.cut.slices, Op = pl.Op;
  TDN_LAUNCH(pred_wgrad_finalize_kernel, dim3(tdn_grid_1d((int64_t)5 * A * C, NT, 4096)), dim3(NT), 0, stream, p, slices, Op,
             dw_cls, dbias_cls, dw_reg, dbias_reg);
  TDN_LAUNCH_CHECK();
  return 0;
}
