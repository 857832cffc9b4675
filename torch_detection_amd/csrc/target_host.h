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
