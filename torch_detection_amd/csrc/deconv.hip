// 2x2 stride-2 transposed convolution: the mask head's upsampling layer as one MFMA GEMM family on the
// core it shares with csrc/linear.hip (csrc/gemm128_core.h: 128 x 128 x 64 tiles, the two-slot LDS ring fed by LDS-DMA,
// the XOR swizzles, both MFMA loops, the split rule).  This file supplies the tap gather of its loaders and its epilogues.
//
// The four taps of a 2x2 stride-2 transposed conv do not overlap:
//     y[r][2i+a][2j+b][o] = act(bias[o] + sum_c x[r][i][j][c] * W[c][o][a][b])
// so with m = (r * H + i) * W + j an input pixel, n = (a * 2 + b) * Cout + o a GEMM column and
// pix(m, a, b) = 4m - 2j + a * 2W + b the output pixel of tap (a, b) of input pixel m:
//
//   forward   Y[m][n]   = x[M][Cin] . w_fwd[4 Cout][Cin]^T, row m / column n stored at y[pix(m, a, b)][o]   (scatter)
//   dgrad     dx[m][c]  = G[M][4 Cout] . w_dgrad[Cin][4 Cout]^T with G[m][n] = g[pix(m, a, b)][o]           (gather)
//   wgrad     dW[n][c]  = sum_m G[m][n] * x[m][c], stored at dw[c][o][a][b];  dbias[o] = sum over the taps of the
//             column sums of G                                                                             (gather)
//
// Cout is a multiple of 64, so a 64-column group of n — one reduction chunk of the dgrad, one LDS-DMA piece of the wgrad,
// four consecutive accumulator columns of the forward — lies inside one tap: the scatter / gather is a per-row, per-chunk
// source or destination pointer and costs no extra pass over the largest tensor of the head.
//
// Forward and dgrad are one launch each.  The weight gradient cuts its reduction over the pixels as linear_wgrad_kernel
// does: every workgroup stores an fp32 partial slab into the caller's workspace with plain stores and a finalize launch
// adds the slabs in slice order, folds the four tap sums into dbias and writes dw in the parameter's own layout.  No
// workgroup waits for another one, there are no counters, no atomics and no memset: the same bits on every run.
#include "gemm128_core.h"

namespace {

constexpr int64_t MAX_PIX = (int64_t)1 << 29, MAX_OUT = (int64_t)1 << 31;
constexpr int MAX_C = 1 << 16;

// output pixel of tap (0, 0) of input pixel m, in pixels of the (R, 2H, 2W) map
__device__ __forceinline__ int64_t pix0(int m, int W) { return 4 * m - 2 * (m % W); }   // 4M < 2^31 (checked on the host)
// offset of tap t = a * 2 + b from tap (0, 0), in pixels
__device__ __forceinline__ int tap_off(int t, int W) { return (t >> 1) * 2 * W + (t & 1); }

// ---- forward / dgrad: C[m][n] = sum_k A[m][k] * B[n][k] -----------------------------------------------------------------
struct DcArgs {
  const bf16_t* A;                 // forward: x [M][Cin];  dgrad: g [4M][Cout], rows gathered per reduction chunk
  const bf16_t* B; int64_t ldb; int b_rows;   // rows n >= b_rows are read from the zero page
  int M, N;                        // input pixels; output columns (forward 4 Cout, dgrad Cin)
  int W, Cin, Cout;
  int nchunks, tiles_n;
  bf16_t* out;                     // forward: y [4M][Cout] (scattered);  dgrad: dx [M][Cin]
  const float* bias; int relu;
};

template <bool F16, bool DGRAD>
__global__ __launch_bounds__(NT) void deconv_gemm_kernel(const DcArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = (int)blockIdx.x;
  const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- loader: dgrad gathers a row of A from the output pixel of the chunk's tap; a row past its operand reads the zero page
  const int lrow = lane >> 3;
  const int src_el = kc_src_el(lane, lrow);
  const bf16_t* const zero = (const bf16_t*)g_zero_page + src_el;
  const bf16_t* a_src[4];
  const bf16_t* b_src[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = kc_row(it, wave, lrow);
    const int m = m0 + row;
    if (m < p.M) a_src[it] = DGRAD ? p.A + pix0(m, p.W) * p.Cout + src_el : p.A + (int64_t)m * p.Cin + src_el;
    else a_src[it] = nullptr;
    b_src[it] = (n0 + row < p.b_rows) ? p.B + (int64_t)(n0 + row) * p.ldb + src_el : nullptr;
  }
  auto stage_load = [&](int chunk, int s) {
    char* sA = smem + s * STAGE;
    char* sB = sA + TILE_BYTES;
    const int k0 = chunk * BK;
    const bool in = chunk < p.nchunks;              // past the end: the zero page (keeps the vmcnt bookkeeping uniform)
    int64_t a_k = k0;                               // forward: column k0 of the row
    if (DGRAD) {                                    // dgrad: channels k0 % Cout .. + 63 of the output pixel of tap k0 / Cout
      const int t = k0 / p.Cout;
      a_k = (int64_t)tap_off(t, p.W) * p.Cout + (k0 - t * p.Cout);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) glds16_async((in && a_src[it]) ? a_src[it] + a_k : zero, sA + kc_dst(it, wave));
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

  kc_ring<F16>(smem, 0, p.nchunks, stage_load, a_off, b_off, k_off, acc);   // nchunks >= 1

  // ---- store: through LDS (the ring is free now).  Straight from the accumulators a wave instruction would write 32-byte
  // pieces of 16 different rows; staged, every lane stores 16 bytes and 16 lanes the 256 contiguous bytes of one row of
  // the tile — forward: 128 channels of one tap's output pixel (two runs of 64 when Cout == 64).
  constexpr int CROW = BN * 2 + 16;               // row pitch of the staged tile: 16-byte aligned, rows 4 banks apart
  __syncthreads();                                // every wave has read its last fragments
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ml = wm * 64 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nl = wn * 64 + j * 16 + fq * 4;
      f32x4_t v = acc[i][j];
      if (!DGRAD) {                               // n0 + nl < N always: N is a multiple of 256
        const int o = (n0 + nl) % p.Cout;
        if (p.bias) v += *(const f32x4_t*)(p.bias + o);
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
      }
      store4_f32<F16>((bf16_t*)(smem + ml * CROW + nl * 2), v);
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < BM * BN / 8 / NT; ++it) {
    const int piece = it * NT + tid;
    const int ml = piece >> 4, nl = (piece & 15) * 8;
    const int m = m0 + ml, n = n0 + nl;
    if (m >= p.M || n >= p.N) continue;
    const bf16x8_t v = *(const bf16x8_t*)(smem + ml * CROW + nl * 2);
    bf16_t* dst;
    if (DGRAD) {
      dst = p.out + (int64_t)m * p.Cin + n;
    } else {
      const int t = n / p.Cout, o = n - t * p.Cout;
      dst = p.out + (pix0(m, p.W) + tap_off(t, p.W)) * p.Cout + o;
    }
    *(bf16x8_t*)dst = v;
  }
}

// ---- wgrad: slab[slice][n][c] = sum over the slice's pixels m of G[m][n] * x[m][c] --------------------------------------
struct DcWgradArgs {
  const bf16_t* g; const bf16_t* x;
  int M, W, Cin, Cout;
  int cps, tiles_o, ntiles;
  float* dw; float* dbias; float beta;
  float* slab; float* colsum;                 // slab[slice][4 Cout][Cin], colsum[slice][4 Cout]
};

template <bool F16>
__global__ __launch_bounds__(NT) void deconv_wgrad_kernel(const DcWgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slice = (int)blockIdx.x / p.ntiles, tile = (int)blockIdx.x - slice * p.ntiles;
  const int tk = tile / p.tiles_o, to = tile - tk * p.tiles_o;
  const int o0 = to * BM, k0 = tk * BN;         // o0 + 127 < 4 Cout always: 4 Cout is a multiple of 256
  const int N = 4 * p.Cout;
  const int m_begin = slice * p.cps * BK;
  const int m_end = min(p.M, m_begin + p.cps * BK);

  // ---- loader: a lane's 16-byte piece of G lies inside one tap; x columns past Cin and rows >= m_end read the zero page
  const int lrow = lane >> 4, pc = lane & 15;
  const int row0 = tr_row0(wave, lrow);         // + it * 16
  const int src_el = tr_src_el(pc, row0);
  const bf16_t* const zero = (const bf16_t*)g_zero_page + (src_el & 63);
  const bool x_ok = k0 + src_el < p.Cin;
  const int gn = o0 + src_el, gt = gn / p.Cout;
  const bf16_t* const gsrc = p.g + (int64_t)tap_off(gt, p.W) * p.Cout + (gn - gt * p.Cout);
  const bf16_t* const xsrc = p.x + k0 + src_el;
  auto stage_load = [&](int mt, int s) {
    char* sG = smem + s * STAGE;
    char* sX = sG + TILE_BYTES;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int m = mt + it * 16 + row0;
      glds16_async(m < m_end ? gsrc + pix0(m, p.W) * p.Cout : zero, sG + tr_dst(it, wave));
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int m = mt + it * 16 + row0;
      glds16_async((x_ok && m < m_end) ? xsrc + (int64_t)m * p.Cin : zero, sX + tr_dst(it, wave));
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

  // ---- store: a lane holds input channels c .. c + 3 of GEMM column n ----
  const int fr = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = o0 + wm * 64 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = k0 + wn * 64 + j * 16 + grp4 * 4;
      if (c >= p.Cin) continue;
      *(f32x4_t*)(p.slab + ((int64_t)slice * N + n) * p.Cin + c) = acc[i][j];
    }
    if (do_colsum && grp4 == 0) p.colsum[(int64_t)slice * N + n] = acc1[i][0];
  }
}

// dw[c][o][0..3] = beta * old + sum over slices, in slice order, of slab[s][t * Cout + o][c];  dbias[o] = beta * old + the
// four taps' column sums, each summed in slice order, added in tap order.  One thread per (o, c), c fastest.
__global__ __launch_bounds__(NT) void deconv_wgrad_finalize_kernel(const DcWgradArgs p, int slices) {
  const int64_t total = (int64_t)p.Cout * p.Cin;
  const int64_t step = 4 * total;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    const int o = (int)(idx / p.Cin);
    const int c = (int)(idx - (int64_t)o * p.Cin);
    f32x4_t v = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float* s = p.slab + ((int64_t)t * p.Cout + o) * p.Cin + c;
      float a = 0.f;
      if (slices > 0) a = s[0];
      for (int k = 1; k < slices; ++k) a += s[k * step];
      v[t] = a;
    }
    f32x4_t* d = (f32x4_t*)(p.dw + ((int64_t)c * p.Cout + o) * 4);
    if (p.beta != 0.f) v += *d * p.beta;
    *d = v;
    if (c == 0 && p.dbias) {
      float b = 0.f;
      for (int t = 0; t < 4; ++t) {
        float a = 0.f;
        for (int k = 0; k < slices; ++k) {
          const float e = p.colsum[(int64_t)k * 4 * p.Cout + t * p.Cout + o];
          a = k == 0 ? e : a + e;
        }
        b = t == 0 ? a : b + a;
      }
      if (p.beta != 0.f) b += p.dbias[o] * p.beta;
      p.dbias[o] = b;
    }
  }
}

// ---- weight pack ------------------------------------------------------------------------------------------------------
// w_fwd[n][c] and w_dgrad[c][n] for n = (a * 2 + b) * Cout + o: W[c][o][a][b] rounded to the element type.  One thread
// per element of each copy, walking that copy in storage order.
template <bool F16>
__global__ __launch_bounds__(NT) void deconv_pack_kernel(const float* __restrict__ w, int64_t s_c, int64_t s_o, int64_t s_a,
                                                         int64_t s_b, int Cin, int Cout, bf16_t* __restrict__ w_fwd,
                                                         bf16_t* __restrict__ w_dgrad) {
  const int N = 4 * Cout;
  const int64_t total = (int64_t)N * Cin;
  for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
    {
      const int n = (int)(idx / Cin), c = (int)(idx - (int64_t)n * Cin);
      const int t = n / Cout, o = n - t * Cout;
      w_fwd[idx] = f32_to_elem<F16>(w[c * s_c + o * s_o + (t >> 1) * s_a + (t & 1) * s_b]);
    }
    if (w_dgrad) {
      const int c = (int)(idx / N), n = (int)(idx - (int64_t)c * N);
      const int t = n / Cout, o = n - t * Cout;
      w_dgrad[idx] = f32_to_elem<F16>(w[c * s_c + o * s_o + (t >> 1) * s_a + (t & 1) * s_b]);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct DcPlan {
  int tiles_r, tiles_c, tiles, chunks, slices, cps, launches;
  int64_t slab_bytes;
};

inline int wg_chunks(int64_t M) { return (int)((M + BK - 1) / BK); }

int check_shape(const char* who, int kind, int R, int H, int W, int Cin, int Cout, int splits) {
  TDN_CHECK(kind >= 0 && kind <= 2, "%s: kind %d is none of 0 (forward), 1 (dgrad), 2 (wgrad)", who, kind);
  TDN_CHECK(R >= 0, "%s: R=%d is negative", who, R);
  TDN_CHECK(H >= 1 && W >= 1, "%s: H=%d, W=%d must be at least 1", who, H, W);
  TDN_CHECK(Cin >= 64 && Cin <= MAX_C && Cin % 64 == 0, "%s: Cin=%d must be a multiple of 64 in 64..%d (Cin %% 64 != 0?)",
            who, Cin, MAX_C);
  TDN_CHECK(Cout >= 64 && Cout <= MAX_C && Cout % 64 == 0,
            "%s: Cout=%d must be a multiple of 64 in 64..%d (Cout %% 64 != 0?)", who, Cout, MAX_C);
  const int64_t M = (int64_t)R * H * W;
  TDN_CHECK(M < MAX_PIX, "%s: R*H*W=%lld must be below 2^29", who, (long long)M);
  TDN_CHECK(4 * M * Cout < MAX_OUT, "%s: R*2H*2W*Cout=%lld must be below 2^31", who, (long long)(4 * M * Cout));
  TDN_CHECK(M * Cin < MAX_OUT, "%s: R*H*W*Cin=%lld must be below 2^31", who, (long long)(M * Cin));
  int hi = kind == 2 ? wg_chunks(M) : 1;
  if (hi < 1) hi = 1;
  TDN_CHECK(splits >= 0 && splits <= hi, "%s: splits=%d out of range 0..%d", who, splits, hi);
  return 0;
}

// Forward and dgrad are never cut.  The weight gradient is cut by split_rule as csrc/linear.hip's is: a product whose
// tiles already give every CU a workgroup runs as one slice, otherwise the slice count aims at FILL_WGS workgroups with
// at least 4 chunks of 64 pixels per slice.
void make_plan(int kind, int64_t M, int Cin, int Cout, int splits, DcPlan& pl) {
  const int N = 4 * Cout;
  if (kind == 0) { pl.tiles_r = (int)((M + BM - 1) / BM); pl.tiles_c = N / BN; pl.chunks = Cin / BK; }
  else if (kind == 1) { pl.tiles_r = (int)((M + BM - 1) / BM); pl.tiles_c = (Cin + BN - 1) / BN; pl.chunks = N / BK; }
  else { pl.tiles_r = N / BM; pl.tiles_c = (Cin + BN - 1) / BN; pl.chunks = wg_chunks(M); }
  pl.tiles = pl.tiles_r * pl.tiles_c;
  pl.slab_bytes = 0;
  if (kind != 2) {
    pl.slices = 1; pl.cps = pl.chunks;
    pl.launches = M > 0 ? 1 : 0;
    return;
  }
  const Split sp = split_rule(pl.tiles, pl.chunks, splits, FILL_WGS, 4);
  pl.cps = sp.cps;
  pl.slices = sp.slices;                                 // 0 for an empty product: the finalize alone writes beta * old
  pl.launches = (M > 0 ? 1 : 0) + 1;                     // the partial products, the finalize
  pl.slab_bytes = (int64_t)pl.slices * N * Cin * 4;
}

struct DcWs { float* slab; float* colsum; int64_t bytes; };
DcWs ws_layout(int kind, int Cout, const DcPlan& pl, void* base) {
  tdn_carver c{(char*)base, 0};
  DcWs w{nullptr, nullptr, 0};
  if (kind == 2 && pl.slices > 0) {
    w.slab = c.take<float>(pl.slab_bytes / 4);
    w.colsum = c.take<float>((int64_t)pl.slices * 4 * Cout);
  }
  w.bytes = c.off;
  return w;
}

template <bool F16, bool DGRAD>
int launch_gemm(DcArgs& p, const DcPlan& pl, hipStream_t stream) {
  if (tdn_allow_lds<deconv_gemm_kernel<F16, DGRAD>>(LDS_BYTES, "deconv_gemm_kernel") < 0) return -1;
  TDN_LAUNCH((deconv_gemm_kernel<F16, DGRAD>), dim3((unsigned)pl.tiles), dim3(NT), LDS_BYTES, stream, p);
  TDN_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int tdn_pack_deconv2x2_weight(const float* w, int64_t s_c, int64_t s_o, int64_t s_a, int64_t s_b, int Cin,
                                         int Cout, void* w_fwd, void* w_dgrad, int dtype, void* stream) {
  const char* who = "tdn_pack_deconv2x2_weight";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 0, 0, 1, 1, Cin, Cout, 0) != 0) return -1;
  TDN_CHECK(w && w_fwd, "%s: NULL pointer", who);
  TDN_CHECK(aligned(w_fwd, 16) && aligned(w_dgrad, 16), "%s: packed weights must be 16-byte aligned", who);
  const int grid = tdn_grid_1d((int64_t)4 * Cout * Cin, NT, 4096);
  TDN_LAUNCH_T(deconv_pack_kernel, dtype, dim3(grid), dim3(NT), stream, w, s_c, s_o, s_a, s_b, Cin, Cout, (bf16_t*)w_fwd,
               (bf16_t*)w_dgrad);
  TDN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t tdn_deconv2x2_workspace_bytes(int kind, int R, int H, int W, int Cin, int Cout, int splits) {
  if (check_shape("tdn_deconv2x2_workspace_bytes", kind, R, H, W, Cin, Cout, splits) != 0) return -1;
  DcPlan pl;
  make_plan(kind, (int64_t)R * H * W, Cin, Cout, splits, pl);
  return ws_layout(kind, Cout, pl, nullptr).bytes;
}

extern "C" int tdn_deconv2x2_plan(int kind, int R, int H, int W, int Cin, int Cout, int splits, int32_t* out) {
  const char* who = "tdn_deconv2x2_plan";
  if (check_shape(who, kind, R, H, W, Cin, Cout, splits) != 0) return -1;
  TDN_CHECK(out, "%s: NULL out", who);
  DcPlan pl;
  make_plan(kind, (int64_t)R * H * W, Cin, Cout, splits, pl);
  const int64_t ws = ws_layout(kind, Cout, pl, nullptr).bytes;
  write_plan(out, pl.tiles_r, pl.tiles_c, pl.slices, pl.cps, pl.chunks, kind == 2 ? pl.tiles * pl.slices : pl.tiles,
             pl.launches, 0, pl.slab_bytes, ws);
  return 0;
}

extern "C" int tdn_deconv2x2_fwd(const void* x, const void* w_fwd, const float* bias, void* y, int R, int H, int W,
                                 int Cin, int Cout, int relu, int dtype, void* stream) {
  const char* who = "tdn_deconv2x2_fwd";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 0, R, H, W, Cin, Cout, 0) != 0) return -1;
  if (R == 0) return 0;
  TDN_CHECK(x && w_fwd && y, "%s: NULL pointer", who);
  TDN_CHECK(aligned(x, 16) && aligned(w_fwd, 16) && aligned(y, 16) && aligned(bias, 16),
            "%s: x, w_fwd, y and bias must be 16-byte aligned", who);
  const int64_t M = (int64_t)R * H * W;
  DcPlan pl;
  make_plan(0, M, Cin, Cout, 0, pl);
  DcArgs p{};
  p.A = (const bf16_t*)x;
  p.B = (const bf16_t*)w_fwd; p.ldb = Cin; p.b_rows = 4 * Cout;
  p.M = (int)M; p.N = 4 * Cout; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.nchunks = pl.chunks; p.tiles_n = pl.tiles_c;
  p.out = (bf16_t*)y; p.bias = bias; p.relu = relu ? 1 : 0;
  return dtype == TDN_F16 ? launch_gemm<true, false>(p, pl, (hipStream_t)stream)
                          : launch_gemm<false, false>(p, pl, (hipStream_t)stream);
}

extern "C" int tdn_deconv2x2_dgrad(const void* g, const void* w_dgrad, void* dx, int R, int H, int W, int Cin, int Cout,
                                   int dtype, void* stream) {
  const char* who = "tdn_deconv2x2_dgrad";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 1, R, H, W, Cin, Cout, 0) != 0) return -1;
  if (R == 0) return 0;
  TDN_CHECK(g && w_dgrad && dx, "%s: NULL pointer", who);
  TDN_CHECK(aligned(g, 16) && aligned(w_dgrad, 16) && aligned(dx, 16), "%s: g, w_dgrad and dx must be 16-byte aligned", who);
  const int64_t M = (int64_t)R * H * W;
  DcPlan pl;
  make_plan(1, M, Cin, Cout, 0, pl);
  DcArgs p{};
  p.A = (const bf16_t*)g;
  p.B = (const bf16_t*)w_dgrad; p.ldb = 4 * Cout; p.b_rows = Cin;
  p.M = (int)M; p.N = Cin; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.nchunks = pl.chunks; p.tiles_n = pl.tiles_c;
  p.out = (bf16_t*)dx; p.bias = nullptr; p.relu = 0;
  return dtype == TDN_F16 ? launch_gemm<true, true>(p, pl, (hipStream_t)stream)
                          : launch_gemm<false, true>(p, pl, (hipStream_t)stream);
}

extern "C" int tdn_deconv2x2_wgrad(const void* x, const void* g, float* dw, float* dbias, float beta, int R, int H, int W,
                                   int Cin, int Cout, int splits, void* workspace, int64_t workspace_bytes, int dtype,
                                   void* stream) {
  const char* who = "tdn_deconv2x2_wgrad";
  TDN_CHECK_DTYPE(dtype);
  if (check_shape(who, 2, R, H, W, Cin, Cout, splits) != 0) return -1;
  const int64_t M = (int64_t)R * H * W;
  TDN_CHECK(dw && (M == 0 || (x && g)), "%s: NULL pointer", who);
  TDN_CHECK(beta == beta, "%s: beta is NaN", who);
  TDN_CHECK(aligned(dw, 16), "%s: dw must be 16-byte aligned", who);
  TDN_CHECK(M == 0 || (aligned(x, 16) && aligned(g, 16)), "%s: x and g must be 16-byte aligned", who);
  DcPlan pl;
  make_plan(2, M, Cin, Cout, splits, pl);
  const DcWs w = ws_layout(2, Cout, pl, workspace);
  if (w.bytes != 0 && tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  DcWgradArgs p{};
  p.g = (const bf16_t*)g; p.x = (const bf16_t*)x;
  p.M = (int)M; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.cps = pl.cps; p.tiles_o = pl.tiles_r; p.ntiles = pl.tiles;
  p.dw = dw; p.dbias = dbias; p.beta = beta;
  p.slab = w.slab; p.colsum = w.colsum;
  return launch_wgrad<deconv_wgrad_kernel<true>, deconv_wgrad_kernel<false>, deconv_wgrad_finalize_kernel>(
      "deconv_wgrad_kernel", dtype == TDN_F16, pl.tiles * pl.slices, p, (int64_t)Cout * Cin, pl.slices,
      (hipStream_t)stream);
}
