// Host hooks of target.hip for dense_detect.hip (not part of the C ABI of include/tdn.h): the assignment launches of
// tdn_anchor_target — valid flags, allowed_border, the six steps — on a workspace that carries `extra_words` more
// 32-bit words, 8-byte aligned, which the first launch clears to 0 with the column maxima.
#pragma once
#include "common.h"

// bytes of the assignment workspace with `extra_words` cleared words behind the column maxima
int64_t tdn_target_anchor_assign_bytes(int B, int G, int64_t extra_words);
// Checks what tdn_anchor_target checks of these arguments (in the name of `who`), lays the workspace out and enqueues
// the launches; *extra = the cleared words.  0, or -1 / -2 with the error set.
int tdn_target_anchor_assign(const char* who, const float* anchors, int64_t box_stride, const uint8_t* valid,
                             int64_t valid_stride, const float* gt, const int32_t* gt_counts, const int32_t* img_shapes,
                             int B, int N, int G, const tdn_target_config* cfg, int32_t* assigned, void* workspace,
                             int64_t extra_words, uint32_t** extra, void* stream);

// For guided.hip, whose two assign passes read several boxes per location: launch 0 (column maxima <- 0, first indices
// <- INT_MAX, `words` of each) and launch 2b (gt_max_assign_all = 0: box first[b][j] gets j + 1, the highest j wins) of
// the assignment as they stand above; words = B * max(G, 1) <= 64 * TDN_TARGET_MAX_GT.  0, or -1 / -2 with the error set.
int tdn_target_clear(uint32_t* colmax, int* first, int64_t words, void* stream);
int tdn_target_assign_first(const int* first, const int32_t* gt_counts, int B, int N, int G, int32_t* assigned,
                            void* stream);
