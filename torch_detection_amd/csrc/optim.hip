// Fused SGD step: gradient-norm clip, loss unscaling with an overflow check, weight decay, momentum
// (plain / Nesterov) and the parameter update of EVERY parameter of a model in two launches, with no host
// synchronisation and no atomics.
//
//   pass 1  sgd_norm_kernel    one workgroup per norm chunk (NORM_CHUNK elements of one gradient, in storage order):
//                              partial[c] = sum of g^2 in float64.  Thread 0 of workgroup 0 snapshots the loss scale
//                              and the first-step flag, so that pass 2 reads nothing that pass 2 writes.
//   pass 2  sgd_update_kernel  every workgroup sums ALL partials in the same fixed order (S is therefore the same bits
//                              in every workgroup, whatever the grid), derives the norm, the clip coefficient and the
//                              skip decision from S and the snapshot, then walks the update chunks.  Thread 0 of
//                              workgroup 0 writes the observable results and steps the loss-scale state machine.
//
// Item descriptors and both chunk maps live in DEVICE memory (the "table"), built once on the host by tdn_sgd_plan and
// copied once by the caller: ResNet-50-FPN has ~175 parameters, which is more than a 4 KB argument block holds.
//
// Arithmetic: every operation below is one IEEE fp32 operation (this file is built with -ffp-contract=off), the fused
// ones are written as __fmaf_rn — the sequence that is bit-identical to torch.optim.SGD(foreach=False) on the CPU.
#include "common.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int TB = 256;            // threads per workgroup, both passes
constexpr int UPD_CHUNK = 4096;    // elements per update chunk (and floats of the transpose tile: 16 KB of LDS)
constexpr int NORM_CHUNK = 16384;  // elements per norm chunk
constexpr int UPD_GRID_MAX = 2048; // 256 CUs x 8 resident workgroups; the chunks beyond are grid-strided
constexpr int MAX_TAPS = 1024;     // transposed path: taps * 4 input channels must fit the tile

enum { PATH_LINEAR = TDN_SGD_PATH_LINEAR, PATH_TRANSPOSED = TDN_SGD_PATH_TRANSPOSED, PATH_GENERAL = TDN_SGD_PATH_GENERAL };

struct DevItem {
  float* p;
  const float* g;
  float* buf;            // NULL: no momentum buffer (the group's momentum is 0)
  int shape[4];
  long long ps[4], gs[4];   // element strides of p (and buf) / of g; used by the general path only
  int group;
  int path;
  int vec;               // p, g and buf are 16-byte aligned
  int taps, cin;         // transposed path: the per-output-channel block is taps x cin
  int numel;
};
struct UpdChunk { int item, a, b, c; };   // linear / general: a = first element, b = count;  transposed: a = output
                                          // channel, b = first input channel, c = input channels
struct NormChunk { int item, off; };

struct Table {
  DevItem* items;
  NormChunk* norm;
  UpdChunk* upd;
  int64_t bytes;
};
// the one layout of the device table (size query with a null base, fill / launch with a pointer)
Table table_layout(int64_t n_items, int64_t n_norm, int64_t n_upd, void* base) {
  tdn_carver c{(char*)base, 0};
  Table t;
  t.items = c.take<DevItem>(n_items);
  t.norm = c.take<NormChunk>(n_norm);
  t.upd = c.take<UpdChunk>(n_upd);
  t.bytes = c.off;
  return t;
}
struct SgdWs { double* partials; int64_t bytes; };
SgdWs ws_layout(int64_t n_norm, void* base) {
  tdn_carver c{(char*)base, 0};
  return {c.take<double>(n_norm), c.off};
}

// ---- device -----------------------------------------------------------------------------------------------------------
// The tensors' pointers come out of the table, so the compiler cannot know their address space and would emit flat
// loads and stores; they are global memory, and saying so gives global_load / global_store.
typedef TDN_GLOBAL float gfloat;
typedef TDN_GLOBAL f32x4_t gfloat4;
__device__ __forceinline__ gfloat* as_global(const float* p) { return (gfloat*)p; }

// sum of the workgroup's values in a fixed order; the result is returned to every thread
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int w = TB / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] = red[tid] + red[tid + w];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(TB) void sgd_norm_kernel(const DevItem* __restrict__ items, const NormChunk* __restrict__ chunks,
                                                      double* __restrict__ partials, float* fstate, int* istate) {
  __shared__ double red[TB];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) {
    fstate[TDN_SGD_F_SNAP_SCALE] = fstate[TDN_SGD_F_SCALE];
    istate[TDN_SGD_I_SNAP_FIRST] = istate[TDN_SGD_I_BUF_INIT] ? 0 : 1;
  }
  const NormChunk ch = chunks[blockIdx.x];
  const DevItem& it = items[ch.item];
  const gfloat* g = as_global(it.g) + ch.off;
  const int rest = it.numel - ch.off;
  const int len = rest < NORM_CHUNK ? rest : NORM_CHUNK;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int done = 0;
  if (it.vec) {   // ch.off is a multiple of NORM_CHUNK: the chunk starts 16-byte aligned
    const int n4 = len >> 2;
    for (int i = tid; i < n4; i += TB) {
      const f32x4_t v = *(const gfloat4*)(g + 4 * i);
      a0 += (double)v[0] * (double)v[0];
      a1 += (double)v[1] * (double)v[1];
      a2 += (double)v[2] * (double)v[2];
      a3 += (double)v[3] * (double)v[3];
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < len; i += TB) a0 += (double)g[i] * (double)g[i];
  const double s = block_sum((a0 + a1) + (a2 + a3), red);
  if (tid == 0) partials[blockIdx.x] = s;
}

struct Coef {
  float m, lr, wd, mom;
  int first, nesterov;
};
// one element: returns the new parameter, b becomes the new momentum value (read only when has_buf)
template <bool HAS_BUF>
__device__ __forceinline__ float sgd_elem(float g, float p, float& b, const Coef& k) {
  const float gh = g * k.m;
  const float d = k.wd != 0.f ? __fmaf_rn(k.wd, p, gh) : gh;
  float u = d;
  if (HAS_BUF) {
    b = k.first ? d : (b * k.mom) + d;
    u = k.nesterov ? __fmaf_rn(k.mom, b, d) : b;
  }
  return __fmaf_rn(-k.lr, u, p);
}

// n consecutive elements of g, p and buf (same element order in all three), from element 0 of the given pointers
template <bool HAS_BUF>
__device__ __forceinline__ void linear_span(const gfloat* __restrict__ g, gfloat* __restrict__ p, gfloat* __restrict__ buf,
                                            int n, bool vec, const Coef& k) {
  const int tid = threadIdx.x;
  int done = 0;
  if (vec) {
    constexpr int U = UPD_CHUNK / (4 * TB);   // 4 float4 per thread, loads first
    const int n4 = n >> 2;
    f32x4_t vg[U], vp[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * TB;
      if (i < n4) {
        vg[u] = *(const gfloat4*)(g + 4 * i);
        vp[u] = *(const gfloat4*)(p + 4 * i);
        if (HAS_BUF) vb[u] = *(const gfloat4*)(buf + 4 * i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * TB;
      if (i < n4) {
        f32x4_t np, nb = vb[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float b = HAS_BUF ? nb[e] : 0.f;
          np[e] = sgd_elem<HAS_BUF>(vg[u][e], vp[u][e], b, k);
          nb[e] = b;
        }
        *(gfloat4*)(p + 4 * i) = np;
        if (HAS_BUF) *(gfloat4*)(buf + 4 * i) = nb;
      }
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < n; i += TB) {
    float b = HAS_BUF ? buf[i] : 0.f;
    p[i] = sgd_elem<HAS_BUF>(g[i], p[i], b, k);
    if (HAS_BUF) buf[i] = b;
  }
}

// Reducer pair: p (and buf) [cin][taps] and g [taps][cin] are transposes of one block per output channel.  The chunk's
// g columns [ci0, ci0 + cb) are read along cin into the tile, p and buf are walked along taps and pick g from the tile.
template <bool HAS_BUF>
__device__ __forceinline__ void transposed_chunk(const DevItem& it, const UpdChunk& ch, float* tile, const Coef& k) {
  const int tid = threadIdx.x;
  const int taps = it.taps, cin = it.cin, ci0 = ch.b, cb = ch.c;
  const long long base = (long long)ch.a * taps * cin;
  const gfloat* g = as_global(it.g) + base + ci0;
  const int n = taps * cb;
  if (it.vec && ((cin | cb | ci0) & 3) == 0) {
    for (int i = 4 * tid; i < n; i += 4 * TB) {
      const int t = i / cb, c = i - t * cb;
      *(f32x4_t*)(tile + i) = *(const gfloat4*)(g + (long long)t * cin + c);
    }
  } else {
    for (int i = tid; i < n; i += TB) {
      const int t = i / cb, c = i - t * cb;
      tile[i] = g[(long long)t * cin + c];
    }
  }
  __syncthreads();
  const long long pbase = base + (long long)ci0 * taps;
  gfloat* p = as_global(it.p) + pbase;
  gfloat* buf = HAS_BUF ? as_global(it.buf) + pbase : nullptr;
  int done = 0;
  if (it.vec && (pbase & 3) == 0) {
    const int n4 = n >> 2;
    for (int i = tid; i < n4; i += TB) {
      int c = (4 * i) / taps, t = 4 * i - c * taps;
      const f32x4_t vp = *(const gfloat4*)(p + 4 * i);
      f32x4_t np, nb;
      if (HAS_BUF) nb = *(const gfloat4*)(buf + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float b = HAS_BUF ? nb[e] : 0.f;
        np[e] = sgd_elem<HAS_BUF>(tile[t * cb + c], vp[e], b, k);
        nb[e] = b;
        if (++t == taps) { t = 0; ++c; }
      }
      *(gfloat4*)(p + 4 * i) = np;
      if (HAS_BUF) *(gfloat4*)(buf + 4 * i) = nb;
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < n; i += TB) {
    const int c = i / taps, t = i - c * taps;
    float b = HAS_BUF ? buf[i] : 0.f;
    p[i] = sgd_elem<HAS_BUF>(tile[t * cb + c], p[i], b, k);
    if (HAS_BUF) buf[i] = b;
  }
  __syncthreads();   // the tile is rewritten by this workgroup's next chunk
}

// any other dense permutation: logical (row-major) element l of the 4-D shape, addressed through both stride sets
template <bool HAS_BUF>
__device__ __forceinline__ void general_chunk(const DevItem& it, const UpdChunk& ch, const Coef& k) {
  for (int e = threadIdx.x; e < ch.b; e += TB) {
    int l = ch.a + e;
    const int i3 = l % it.shape[3]; l /= it.shape[3];
    const int i2 = l % it.shape[2]; l /= it.shape[2];
    const int i1 = l % it.shape[1];
    const int i0 = l / it.shape[1];
    const long long po = i0 * it.ps[0] + i1 * it.ps[1] + i2 * it.ps[2] + i3 * it.ps[3];
    const long long go = i0 * it.gs[0] + i1 * it.gs[1] + i2 * it.gs[2] + i3 * it.gs[3];
    gfloat* p = as_global(it.p) + po;
    gfloat* buf = as_global(it.buf) + po;
    float b = HAS_BUF ? *buf : 0.f;
    *p = sgd_elem<HAS_BUF>(as_global(it.g)[go], *p, b, k);
    if (HAS_BUF) *buf = b;
  }
}

template <bool HAS_BUF>
__device__ __forceinline__ void run_chunk(const DevItem& it, const UpdChunk& ch, float* tile, const Coef& k) {
  if (it.path == PATH_LINEAR)
    linear_span<HAS_BUF>(as_global(it.g) + ch.a, as_global(it.p) + ch.a, HAS_BUF ? as_global(it.buf) + ch.a : nullptr,
                         ch.b, it.vec != 0, k);
  else if (it.path == PATH_TRANSPOSED)
    transposed_chunk<HAS_BUF>(it, ch, tile, k);
  else
    general_chunk<HAS_BUF>(it, ch, k);
}

struct StepArgs {
  const DevItem* items;
  const UpdChunk* chunks;
  const double* partials;
  const float* hyper;    // [groups][3] = lr, weight decay, momentum
  float* fstate;
  int* istate;
  int nchunks, npartials;
  int nesterov, skip, dynamic;
  float max_norm, growth, backoff;
  int interval;
};

__global__ __launch_bounds__(TB) void sgd_update_kernel(const StepArgs A) {
  __shared__ double red[TB];
  __shared__ __attribute__((aligned(16))) float tile[UPD_CHUNK];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < A.npartials; i += TB) s += A.partials[i];
  const double S = block_sum(s, red);
  const bool finite = __builtin_isfinite(S);
  const float scale = A.fstate[TDN_SGD_F_SNAP_SCALE];
  const int first = A.istate[TDN_SGD_I_SNAP_FIRST];
  const float inv = 1.0f / scale;
  const float n = (float)(sqrt(S) * (double)inv);
  float coef = 1.0f;
  if (A.max_norm > 0.f) {
    const float c = A.max_norm / (n + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;     // a NaN stays a NaN, as torch.clamp(max=1) leaves it
  }
  const bool skipped = A.skip && !finite;
  if (blockIdx.x == 0 && tid == 0) {
    A.fstate[TDN_SGD_F_NORM] = n;
    A.fstate[TDN_SGD_F_COEF] = coef;
    if (A.dynamic) {   // torch._amp_update_scale_
      if (!finite) {
        A.fstate[TDN_SGD_F_SCALE] = scale * A.backoff;
        A.istate[TDN_SGD_I_TRACKER] = 0;
      } else {
        const int ok = A.istate[TDN_SGD_I_TRACKER] + 1;
        if (ok == A.interval) {
          const float grown = scale * A.growth;
          if (__builtin_isfinite(grown)) A.fstate[TDN_SGD_F_SCALE] = grown;
          A.istate[TDN_SGD_I_TRACKER] = 0;
        } else {
          A.istate[TDN_SGD_I_TRACKER] = ok;
        }
      }
    }
    if (skipped) {
      A.istate[TDN_SGD_I_SKIPPED] += 1;
    } else {
      A.istate[TDN_SGD_I_TAKEN] += 1;
      A.istate[TDN_SGD_I_BUF_INIT] = 1;
    }
    A.istate[TDN_SGD_I_LAST_SKIPPED] = skipped ? 1 : 0;
  }
  if (skipped) return;   // p and buf keep their bits
  Coef k;
  k.m = coef * inv;
  k.first = first;
  k.nesterov = A.nesterov;
  for (int c = blockIdx.x; c < A.nchunks; c += gridDim.x) {
    const UpdChunk ch = A.chunks[c];
    const DevItem& it = A.items[ch.item];
    const float* h = A.hyper + 3 * it.group;
    k.lr = h[0];
    k.wd = h[1];
    k.mom = h[2];
    if (it.buf) run_chunk<true>(it, ch, tile, k);
    else run_chunk<false>(it, ch, tile, k);
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
// dims of size > 1 sorted by stride must tile a dense block: stride[k] = product of the sizes below it
bool dense_nonoverlapping(const int64_t* shape, const int64_t* st) {
  int idx[4], n = 0;
  for (int d = 0; d < 4; ++d)
    if (shape[d] > 1) idx[n++] = d;
  for (int a = 1; a < n; ++a)
    for (int b = a; b > 0 && st[idx[b]] < st[idx[b - 1]]; --b) { const int t = idx[b]; idx[b] = idx[b - 1]; idx[b - 1] = t; }
  int64_t want = 1;
  for (int a = 0; a < n; ++a) {
    if (st[idx[a]] != want) return false;
    want *= shape[idx[a]];
  }
  return true;
}

int classify(const tdn_sgd_item& s) {
  bool same = true;
  for (int d = 0; d < 4; ++d)
    if (s.shape[d] > 1 && s.p_stride[d] != s.g_stride[d]) same = false;
  if (same) return PATH_LINEAR;
  const int64_t O = s.shape[0], I = s.shape[1], kh = s.shape[2], kw = s.shape[3], T = kh * kw;
  auto is = [&](const int64_t* st, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
    return (O == 1 || st[0] == s0) && (I == 1 || st[1] == s1) && (kh == 1 || st[2] == s2) && (kw == 1 || st[3] == s3);
  };
  if (I > 1 && T > 1 && T <= MAX_TAPS && is(s.p_stride, I * T, T, kw, 1) && is(s.g_stride, T * I, 1, kw * I, I))
    return PATH_TRANSPOSED;
  return PATH_GENERAL;
}

int check_item(const char* who, const tdn_sgd_item& s, int i, int n_groups, int64_t* numel) {
  TDN_CHECK(s.p && s.g, "%s: item %d: NULL parameter or gradient pointer", who, i);
  TDN_CHECK(s.group >= 0 && s.group < n_groups, "%s: item %d: group %d out of 0..%d", who, i, s.group, n_groups - 1);
  int64_t n = 1;
  for (int d = 0; d < 4; ++d) {
    TDN_CHECK(s.shape[d] >= 1 && s.shape[d] < (1ll << 31), "%s: item %d: shape[%d]=%lld", who, i, d, (long long)s.shape[d]);
    n *= s.shape[d];
    TDN_CHECK(n < (1ll << 31), "%s: item %d holds 2^31 elements or more", who, i);
  }
  TDN_CHECK(dense_nonoverlapping(s.shape, s.p_stride), "%s: item %d: the parameter is not a dense, non-overlapping tensor", who, i);
  TDN_CHECK(dense_nonoverlapping(s.shape, s.g_stride), "%s: item %d: the gradient is not a dense, non-overlapping tensor", who, i);
  TDN_CHECK(((uintptr_t)s.p & 3) == 0 && ((uintptr_t)s.g & 3) == 0 && ((uintptr_t)s.buf & 3) == 0,
            "%s: item %d: pointers must be 4-byte aligned", who, i);
  *numel = n;
  return 0;
}

}  // namespace

extern "C" int tdn_sgd_plan(const tdn_sgd_item* items, int n, int n_groups, int64_t* plan8, void* table_host,
                            int64_t table_bytes, int32_t* paths) {
  const char* who = "tdn_sgd_plan";
  TDN_CHECK(items && n >= 1 && n <= TDN_SGD_MAX_ITEMS, "%s: %d items (1..%d)", who, n, TDN_SGD_MAX_ITEMS);
  TDN_CHECK(n_groups >= 1 && n_groups <= TDN_SGD_MAX_GROUPS, "%s: %d groups (1..%d)", who, n_groups, TDN_SGD_MAX_GROUPS);
  TDN_CHECK(plan8, "%s: NULL plan", who);
  // first walk: counts
  int64_t n_norm = 0, n_upd = 0;
  for (int i = 0; i < n; ++i) {
    int64_t numel;
    if (check_item(who, items[i], i, n_groups, &numel) != 0) return -1;
    n_norm += (numel + NORM_CHUNK - 1) / NORM_CHUNK;
    const int path = classify(items[i]);
    if (path == PATH_TRANSPOSED) {
      const int64_t T = items[i].shape[2] * items[i].shape[3], I = items[i].shape[1];
      const int64_t cb = T * I <= UPD_CHUNK ? I : (UPD_CHUNK / T) & ~3ll;
      n_upd += items[i].shape[0] * ((I + cb - 1) / cb);
    } else {
      n_upd += (numel + UPD_CHUNK - 1) / UPD_CHUNK;
    }
    if (paths) paths[i] = path;
  }
  TDN_CHECK(n_norm < (1ll << 24) && n_upd < (1ll << 28), "%s: too many chunks", who);
  const Table size = table_layout(n, n_norm, n_upd, nullptr);
  plan8[0] = size.bytes;
  plan8[1] = ws_layout(n_norm, nullptr).bytes;
  plan8[2] = n_norm;                                          // workgroups of pass 1
  plan8[3] = n_upd < UPD_GRID_MAX ? n_upd : UPD_GRID_MAX;     // workgroups of pass 2
  plan8[4] = n_norm;
  plan8[5] = n_upd;
  plan8[6] = n;
  plan8[7] = n_groups;
  if (!table_host) return 0;
  TDN_CHECK(((uintptr_t)table_host & 15) == 0, "%s: the table buffer must be 16-byte aligned", who);
  TDN_CHECK(table_bytes >= size.bytes, "%s: the table buffer holds %lld bytes, %lld are needed", who,
            (long long)table_bytes, (long long)size.bytes);
  memset(table_host, 0, (size_t)size.bytes);
  const Table t = table_layout(n, n_norm, n_upd, table_host);
  int64_t cn = 0, cu = 0;
  for (int i = 0; i < n; ++i) {
    const tdn_sgd_item& s = items[i];
    DevItem& d = t.items[i];
    int64_t numel = 1;
    for (int k = 0; k < 4; ++k) {
      d.shape[k] = (int)s.shape[k];
      d.ps[k] = s.shape[k] > 1 ? s.p_stride[k] : 0;
      d.gs[k] = s.shape[k] > 1 ? s.g_stride[k] : 0;
      numel *= s.shape[k];
    }
    d.p = s.p; d.g = s.g; d.buf = s.buf;
    d.group = s.group;
    d.path = classify(s);
    d.vec = (((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.buf) & 15) == 0;
    d.numel = (int)numel;
    for (int64_t off = 0; off < numel; off += NORM_CHUNK) t.norm[cn++] = {i, (int)off};
    if (d.path == PATH_TRANSPOSED) {
      d.taps = (int)(s.shape[2] * s.shape[3]);
      d.cin = (int)s.shape[1];
      const int cb = d.taps * d.cin <= UPD_CHUNK ? d.cin : (UPD_CHUNK / d.taps) & ~3;
      for (int o = 0; o < d.shape[0]; ++o)
        for (int c0 = 0; c0 < d.cin; c0 += cb) t.upd[cu++] = {i, o, c0, d.cin - c0 < cb ? d.cin - c0 : cb};
    } else {
      for (int64_t off = 0; off < numel; off += UPD_CHUNK)
        t.upd[cu++] = {i, (int)off, (int)(numel - off < UPD_CHUNK ? numel - off : UPD_CHUNK), 0};
    }
  }
  TDN_CHECK(cn == n_norm && cu == n_upd, "%s: internal: chunk counts disagree", who);
  return 0;
}

extern "C" int tdn_sgd_step(const void* table, const int64_t* plan8, const float* hyper, float* fstate, int32_t* istate,
                            void* workspace, int64_t workspace_bytes, int flags, float max_norm, float growth,
                            float backoff, int interval, void* stream) {
  const char* who = "tdn_sgd_step";
  TDN_CHECK(table && plan8 && hyper && fstate && istate, "%s: NULL pointer", who);
  const int64_t n_norm = plan8[4], n_upd = plan8[5], n = plan8[6];
  TDN_CHECK(n >= 1 && n <= TDN_SGD_MAX_ITEMS && n_norm >= 1 && n_norm < (1ll << 24) && n_upd >= 1 && n_upd < (1ll << 28) &&
                plan8[2] == n_norm && plan8[3] == (n_upd < UPD_GRID_MAX ? n_upd : UPD_GRID_MAX),
            "%s: not a plan of tdn_sgd_plan", who);
  TDN_CHECK(((uintptr_t)table & 255) == 0, "%s: the table must be 256-byte aligned", who);
  TDN_CHECK((flags & ~(TDN_SGD_NESTEROV | TDN_SGD_SKIP_NONFINITE | TDN_SGD_DYNAMIC_SCALE)) == 0, "%s: unknown flags %d", who, flags);
  TDN_CHECK(!(max_norm != max_norm), "%s: max_norm is NaN", who);
  if (flags & TDN_SGD_DYNAMIC_SCALE)
    TDN_CHECK(growth > 1.f && backoff > 0.f && backoff < 1.f && interval >= 1,
              "%s: dynamic loss scale needs growth > 1, 0 < backoff < 1, interval >= 1", who);
  const SgdWs w = ws_layout(n_norm, workspace);
  if (tdn_check_ws(who, workspace, workspace_bytes, w.bytes) != 0) return -1;
  const Table t = table_layout(n, n_norm, n_upd, (void*)table);
  TDN_LAUNCH(sgd_norm_kernel, dim3((unsigned)n_norm), dim3(TB), 0, stream, (const DevItem*)t.items,
             (const NormChunk*)t.norm, w.partials, fstate, (int*)istate);
  TDN_LAUNCH_CHECK();
  StepArgs A;
  A.items = t.items;
  A.chunks = t.upd;
  A.partials = w.partials;
  A.hyper = hyper;
  A.fstate = fstate;
  A.istate = (int*)istate;
  A.nchunks = (int)n_upd;
  A.npartials = (int)n_norm;
  A.nesterov = (flags & TDN_SGD_NESTEROV) ? 1 : 0;
  A.skip = (flags & TDN_SGD_SKIP_NONFINITE) ? 1 : 0;
  A.dynamic = (flags & TDN_SGD_DYNAMIC_SCALE) ? 1 : 0;
  A.max_norm = max_norm;
  A.growth = growth;
  A.backoff = backoff;
  A.interval = interval;
  TDN_LAUNCH(sgd_update_kernel, dim3((unsigned)plan8[3]), dim3(TB), 0, stream, A);
  TDN_LAUNCH_CHECK();
  return 0;
}
