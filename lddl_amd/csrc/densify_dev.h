// The dense packing of the kept tokens, one wave's share (densify_group): called by the kernels
// of pairs_densify.hip and by plan_replay_kernel's dense-packing workgroups (pairs.hip). Each
// translation unit gets its own copy (anonymous namespace).
#pragma once
#include "pairs_plan.h"

namespace lddl {
namespace {

// Kept tokens packed densely (see densify_kernel, pairs_densify.hip):
// one wave: kept sentences [k0, k0 + 64)
__device__ inline void densify_group(int64_t k0, const int64_t* __restrict__ ks_start,
                                     const int32_t* __restrict__ ks_len,
                                     const int64_t* __restrict__ kscan, int64_t n,
                                     const int32_t* __restrict__ ids, IdPtr dense) {
  const int lane = threadIdx.x & 63;
  const int64_t k = k0 + lane;
  const bool ok = k < n;
  const int32_t len = ok ? ks_len[k] & kLenMask : 0;
  const int64_t st = ok ? ks_start[k] : 0;
  const int32_t incl = wave_incl_scan(len);
  const int32_t total = __builtin_amdgcn_readlane(incl, 63);  // (uniform: scalar loop bounds)
  const int64_t base = kscan[k0];
  // the sentence loop indices are wave-uniform: lane values via readlane, not LDS permutes
  auto rl = [](int32_t v, int i) { return __builtin_amdgcn_readlane(v, i); };
  // kU chunks of 64 tokens per round: their sources first, then all kU loads, then the stores,
  // so a wave has kU loads in flight instead of one dependent load -> store per chunk
  constexpr int kU = 4;  // (8: 6.0 -> 6.3 ms, profiles/r06y)
  int j = 0;
  for (int32_t c0 = 0; c0 < total; c0 += 64 * kU) {
    int64_t src[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int32_t cu = c0 + 64 * u, x = cu + lane, hi = min(cu + 63, total - 1);
      src[u] = 0;
      if (cu < total) {
        while (rl(incl, j) <= cu) ++j;  // first sentence overlapping the chunk
        for (int jj = j;; ++jj) {
          const int32_t e = rl(incl, jj);
          const int32_t b = e - rl(len, jj);
          const int64_t s = ((int64_t)rl((int32_t)(st >> 32), jj) << 32) | (uint32_t)rl((int32_t)st, jj);
          if (x >= b && x < e) src[u] = s + (x - b);
          if (e > hi) break;
        }
      }
    }
    int32_t v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) v[u] = c0 + 64 * u + lane < total ? ids[src[u]] : 0;
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (c0 + 64 * u + lane < total) dense.st(base + c0 + 64 * u + lane, v[u]);
  }
}

}  // namespace
}  // namespace lddl
