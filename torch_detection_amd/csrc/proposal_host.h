// Host hooks of proposal.hip for guided.hip (not part of the C ABI of include/tdn.h): the workspace of
// tdn_rpn_proposals and its launches 2-4 — suppression words, keep scan, per-image merge — on segments that another
// first launch has filled.  Both hooks run tdn_rpn_proposals' own plan (its checks and limits, in its name) on `levels`.
#pragma once
#include "common.h"

// The regions of tdn_rpn_proposals' workspace.  Segment s = b * nlevels + l owns rows [seg_start[s], + cap_l) with
// seg_start[s] = b * (sum of cap) + (sum of cap below l), cap_l = nms_pre > 0 ? min(n_l, nms_pre) : n_l.  Launch 1 writes
// seg_box / seg_key (order_key of the logit) / seg_aidx (row of the concatenated pyramid) of the segment's rows in key
// order, compacted, and seg_start[s], seg_count[s].
struct tdn_rpn_ws {
  f32x4_t* seg_box;
  uint32_t* seg_key;
  int* seg_aidx;
  int64_t* kept;
  int *seg_start, *seg_count, *num_kept;
  unsigned long long* mask;
  int64_t bytes;
};
// base == nullptr: the size query.  0, or -1 with the error set.
int tdn_rpn_ws_layout(const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg, void* base,
                      tdn_rpn_ws* out);
// launches 2-4 of tdn_rpn_proposals.  0, or -1 / -2 with the error set.
int tdn_rpn_nms_merge(const tdn_rpn_level* levels, int nlevels, int B, const tdn_rpn_config* cfg, const tdn_rpn_ws* w,
                      float* proposals, int64_t* anchor_idx, int32_t* counts, void* stream);
