// RoBERTa blocks: what the plan (blocks_plan.hip) and the collate
// (blocks_collate.hip) share: the tile of the two-level pointer jump, the cap of the collate's
// LDS table, and the cost of a sentence. include/lddl_amd.h states the semantics.
#pragma once
#include "device.h"
#include "lddl_amd.h"

namespace lddl {

constexpr int kBlkTile = LDDL_BLOCKS_TILE;  // sentences per workgroup of the tile and mark passes
constexpr int kBlkThreads = 256;
constexpr int kBlkItems = kBlkTile / kBlkThreads;
constexpr int kBlkLdsSents = LDDL_BLOCKS_LDS_SENTS;  // sentences of a block the collate stages

constexpr int log2_ceil(int v) { return v <= 1 ? 0 : 1 + log2_ceil((v + 1) / 2); }
// a chain inside a tile has at most kBlkTile - 1 jumps: that many doublings reach its end
constexpr int kBlkRounds = log2_ceil(kBlkTile);

static_assert(kBlkTile >= 1024 && kBlkTile <= 4096 && kBlkTile % kBlkThreads == 0, "tile");

// c(s) = min(len(s) + sep(s), T); the scan's functor, and the oracle's cost
struct BlockCost {
  const int32_t* sent_len;
  const uint8_t* sep;
  int32_t T;
  __device__ int64_t operator()(int64_t s) const {
    const int32_t c = (sent_len[s] & kLenMask) + sep[s];
    return c < T ? c : T;
  }
};

}  // namespace lddl
