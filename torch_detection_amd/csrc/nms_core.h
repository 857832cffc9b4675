// Device pieces of greedy NMS shared by tdn_nms (box.hip) and the segmented NMS of proposal.hip: the '+1' IoU, the
// 64x64 suppression-word block and the 1024-thread keep scan.  Both translation units are compiled with
// -ffp-contract=off, so the IoU is the oracle's (oracle/box_ref.c) bit for bit.
#pragma once
#include "common.h"

__device__ __forceinline__ float box_area(const f32x4_t b) {
  return __fmul_rn(__fadd_rn(__fsub_rn(b[2], b[0]), 1.0f), __fadd_rn(__fsub_rn(b[3], b[1]), 1.0f));
}

// IoU of boxes a, b with both areas supplied (box_area is a pure function of its box)
__device__ __forceinline__ float box_iou2(const f32x4_t a, const float area_a, const f32x4_t b, const float area_b) {
  const float ltx = fmaxf(a[0], b[0]), lty = fmaxf(a[1], b[1]);
  const float rbx = fminf(a[2], b[2]), rby = fminf(a[3], b[3]);
  const float w = fmaxf(__fadd_rn(__fsub_rn(rbx, ltx), 1.0f), 0.0f);
  const float h = fmaxf(__fadd_rn(__fsub_rn(rby, lty), 1.0f), 0.0f);
  const float inter = __fmul_rn(w, h);
  const float uni = __fsub_rn(__fadd_rn(area_a, area_b), inter);
  return __fdiv_rn(inter, uni);
}

// 64-bit suppression words of one 64 x 64 block (rb, cb) of N sorted boxes: mask[i * pitch + cb] bit b  <=>
// j = cb*64+b > i  and  iou(i, j) > thr.  One wave: lane l owns COLUMN box j = cb*64 + l (its area computed once); for
// every row r of the block the 64 predicates of the lanes are gathered into the row's word with a wavefront ballot,
// and lane r keeps it.  Blocks under the diagonal are never read by the scan; callers skip them (cb < rb).
__device__ __forceinline__ void nms_mask_block(const float* __restrict__ sboxes, int N, float thr, int pitch, int rb,
                                               int cb, unsigned long long* __restrict__ mask) {
  __shared__ f32x4_t rbox[64];
  const int t = threadIdx.x;
  const int ir = rb * 64 + t;
  rbox[t] = (ir < N) ? *(const f32x4_t*)(sboxes + (int64_t)ir * 4) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int j = cb * 64 + t;
  const bool jvalid = j < N;
  const f32x4_t bj = jvalid ? *(const f32x4_t*)(sboxes + (int64_t)j * 4) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const float area_j = box_area(bj);
  __syncthreads();
  unsigned long long mine = 0ull;
  const int nrow = min(64, N - rb * 64);
  for (int r = 0; r < nrow; ++r) {
    const int i = rb * 64 + r;
    const f32x4_t bi = rbox[r];                       // LDS broadcast
    const float area_i = box_area(bi);
    // argument order as in the oracle's nms: iou(box_i, box_j)
    const bool hit = jvalid && j > i && box_iou2(bi, area_i, bj, area_j) > thr;
    const unsigned long long word = __ballot(hit);
    mine = (t == r) ? word : mine;
  }
  if (ir < N) mask[(int64_t)ir * pitch + cb] = mine;
}

// Keep scan by a 1024-thread workgroup, in super-chunks of 16 chunks (1024 boxes):
//   A  all threads: the super-chunk's 1024 x 16-word diagonal band of the mask -> LDS (128 KB), one row per thread;
//   B  wave 0: the 16 chunks in order, entirely from LDS.  Resolving a chunk's diagonal word is serial only over the
//      boxes that overlap a LATER box of the same chunk (rows with a non-zero diagonal word — found with one wavefront
//      ballot; a box with an all-zero row suppresses nothing inside the chunk, so its fate is simply its bit once the
//      earlier non-zero rows have been applied): ~1 iteration per chunk on sparse inputs instead of one per kept box.
//      Then keep flags and compacted indices are written (a lane's slot = kept boxes before the chunk + popcount of the
//      kept bits below the lane, i.e. its rank in the ballot), and the kept rows are OR-ed into the removal words of
//      the band's later chunks: lane = (word, quarter of the rows), quarters combined with two wave shuffles;
//   C  all threads: wave w ORs the kept rows of chunk w into the removal words past the band — lanes = consecutive
//      words (coalesced), eight rows in flight — and adds its result to the bitmap with one LDS atomic per word.
// The single-wave kernel of box.hip pays a global-memory round trip per chunk on its critical path (157 at N = 10k) and
// one serial step per kept box; here the serial part touches LDS only and global latency is paid twice per 1024 boxes.
//
// Row i of the mask starts at mask + i * pitch (pitch >= nblk = ceil(N/64)).  order[i] is the caller's index of sorted
// box i; order == nullptr: the index is i itself.  keep (may be nullptr) is indexed by that index; kept_idx[0..N) gets
// the kept indices in sorted order, padded with -1.
constexpr int NMS_SC = 16;                       // chunks per super-chunk
constexpr int NMS_SCROWS = NMS_SC * 64;          // 1024 rows = threads
constexpr int NMS_DPITCH = NMS_SCROWS + 1;       // words; odd pitch: the 16 words of one row sit in 16 different banks
constexpr int NMS_BLOCK_MAX_NBLK = 3000;         // removal bitmap + band must fit 160 KB of LDS

// dynamic LDS bytes of nms_scan_block for `nblk` removal words
__host__ __device__ constexpr size_t nms_scan_block_lds(int nblk) {
  return (size_t)(((nblk + 1) & ~1) + NMS_SC * NMS_DPITCH + NMS_SC) * 8 + NMS_SCROWS * 4;
}

__device__ __forceinline__ void nms_scan_block(const unsigned long long* __restrict__ mask,
                                               const int* __restrict__ order, int N, int nblk, int pitch,
                                               uint8_t* keep, int64_t* kept_idx, int* num_kept,
                                               unsigned long long* sm) {
  unsigned long long* remv = sm;                                  // [nblk]
  unsigned long long* D = sm + ((nblk + 1) & ~1);                 // [NMS_SC][NMS_DPITCH]
  unsigned long long* kbits = D + NMS_SC * NMS_DPITCH;            // [NMS_SC]
  int* ord = (int*)(kbits + NMS_SC);                              // [NMS_SCROWS] original indices of the band's boxes
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int w = tid; w < nblk; w += 1024) remv[w] = 0ull;
  int cnt = 0;                                                    // wave 0 only
  const int nsuper = (nblk + NMS_SC - 1) / NMS_SC;
  for (int s = 0; s < nsuper; ++s) {
    const int c0 = s * NMS_SC;
    const int nch = min(NMS_SC, nblk - c0);
    const int row = c0 * 64 + tid;
    // ---- A: diagonal band -> LDS ----
    // 16 lanes read the 16 words of one row (128 contiguous bytes): a wave instruction covers 4 rows = 4-8 cache
    // lines, not 64 rows of one word each
    {
      const int k = tid & 15;
#pragma unroll 4
      for (int j = 0; j < NMS_SC; ++j) {
        const int r = (tid >> 4) + 64 * j;              // row of the band
        const int grow = c0 * 64 + r;
        unsigned long long v = 0ull;
        if (grow < N && k < nch) v = mask[(int64_t)grow * pitch + c0 + k];
        D[k * NMS_DPITCH + r] = v;
      }
      ord[tid] = (row < N) ? (order ? order[row] : row) : 0;   // no global load is left on wave 0's serial path below
    }
    __syncthreads();
    // ---- B: serial resolution of the band, wave 0 ----
    if (wave == 0) {
      const int tw = lane & 15, part = lane >> 4;     // band OR: target word offset, quarter of the chunk's rows
      for (int kc = 0; kc < nch; ++kc) {
        const int c = c0 + kc;
        const int i = c * 64 + lane;
        const unsigned long long diag = D[kc * NMS_DPITCH + kc * 64 + lane];
        const int nvalid = min(64, N - c * 64);
        unsigned long long alive = ~remv[c];
        if (nvalid < 64) alive &= (1ull << nvalid) - 1ull;
        const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
        unsigned long long todo = alive & __ballot(diag != 0ull);   // boxes that can suppress inside this chunk
        while (todo) {
          const int b = __builtin_ctzll(todo);
          const unsigned lo = __builtin_amdgcn_readlane(dlo, b), hi = __builtin_amdgcn_readlane(dhi, b);
          const unsigned long long rowbits = ((unsigned long long)hi << 32) | lo;   // only bits above b
          alive &= ~rowbits;
          todo &= ~rowbits;
          todo &= todo - 1;                           // b itself is done (and kept)
        }
        const unsigned long long keepbits = alive;
        if (i < N) {
          const bool k = (keepbits >> lane) & 1ull;
          const int oi = ord[kc * 64 + lane];
          if (keep) keep[oi] = k ? 1 : 0;
          if (k) kept_idx[cnt + __builtin_popcountll(keepbits & ((1ull << lane) - 1ull))] = (int64_t)oi;
        }
        cnt += __builtin_popcountll(keepbits);
        if (lane == 0) kbits[kc] = keepbits;
        // kept rows -> removal words of the band's later chunks
        {
          const int k2 = kc + 1 + tw;
          unsigned long long acc = 0ull;
          if (k2 < nch) {
            unsigned long long kb = (keepbits >> (part * 16)) & 0xFFFFull;
            const unsigned long long* col = D + k2 * NMS_DPITCH + kc * 64 + part * 16;
            while (kb) {
              const int b0 = __builtin_ctzll(kb); kb &= kb - 1;
              unsigned long long v0 = col[b0], v1 = 0ull, v2 = 0ull, v3 = 0ull;
              if (kb) { const int b1 = __builtin_ctzll(kb); kb &= kb - 1; v1 = col[b1]; }
              if (kb) { const int b2 = __builtin_ctzll(kb); kb &= kb - 1; v2 = col[b2]; }
              if (kb) { const int b3 = __builtin_ctzll(kb); kb &= kb - 1; v3 = col[b3]; }
              acc |= (v0 | v1) | (v2 | v3);
            }
          }
          acc |= __shfl_xor(acc, 16, 64);
          acc |= __shfl_xor(acc, 32, 64);
          if (part == 0 && k2 < nch && acc) remv[c0 + k2] |= acc;
        }
        __threadfence_block();                        // the removal words written above are read by every lane next round
      }
    }
    __syncthreads();
    // ---- C: kept rows of the band -> removal words past the band ----
    // wave w takes the kept rows of chunk w, lanes take consecutive words (512-byte coalesced reads), sixteen rows in
    // flight per lane; one LDS atomic per lane and word slot at the end
    const int wbeg = c0 + nch;
    if (wbeg < nblk && wave < nch) {
      const unsigned long long keepbits = kbits[wave];
      const unsigned long long* base = mask + (int64_t)(c0 + wave) * 64 * pitch;
      for (int wb = wbeg; wb < nblk; wb += 64) {
        const int w = wb + lane;
        if (w < nblk) {
          unsigned long long acc = 0ull, kb = keepbits;
          while (kb) {
            unsigned long long v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              v[e] = 0ull;
              if (kb) {
                const int b = __builtin_ctzll(kb);
                kb &= kb - 1;
                v[e] = base[(int64_t)b * pitch + w];
              }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc |= v[e];
          }
          if (acc) atomicOr(&remv[w], acc);
        }
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    for (int k = cnt + lane; k < N; k += 64) kept_idx[k] = -1;
    if (lane == 0) *num_kept = cnt;
  }
}
