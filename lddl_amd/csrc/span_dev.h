// N-gram (span) dynamic masking, the device side shared by the collate kernels: the
// span arguments and one 64-slot window of the decision, which a kernel's one word loop calls in
// place of word_masked. The kernels keep their loops and stores (collate_dev.h says
// why); each translation unit gets its own copy (anonymous namespace).
//
// Words are counted over non-special slots; a non-special head h of word j starts a span iff its
// own mask draw says so (u01(r(h).x) < p_start), the span's length in words comes from a second
// Philox call at the same index and counter under the key seed2, and slot x is masked iff the
// furthest reach max_{j' <= word(x)} (j' + len) of the spans started at or before its word lies
// past it: a prefix maximum.
#pragma once
#include "collate_dev.h"

namespace lddl {
namespace {

constexpr int kSpanMaxN = 16;

// (the longest span n is not here: cum[] is 1 from n - 1 on, which is all the device needs)
struct SpanDraw {
  uint64_t seed2;            // seed ^ LDDL_SPAN_SEED_XOR: the key of the length draw
  float p_start;
  float cum[kSpanMaxN - 1];  // cum[k - 1] = P(len <= k) for k < n, 1 from there on
};

// len = 1 + #{k in [1, n) : u >= c_k}; the entries from n - 1 on are 1 > u
__device__ inline int32_t span_len(const SpanDraw& S, uint64_t counter, int64_t flat) {
  const uint4 r2 = Philox::gen(make_uint4((uint32_t)flat, (uint32_t)(flat >> 32),
                                          (uint32_t)counter, (uint32_t)(counter >> 32)),
                               make_uint2((uint32_t)S.seed2, (uint32_t)(S.seed2 >> 32)));
  const float u = u01(r2.x);
  int32_t len = 1;
#pragma unroll
  for (int k = 0; k < kSpanMaxN - 1; ++k) len += u >= S.cum[k] ? 1 : 0;
  return len;
}

// One 64-slot window of a row, lane = slot, EVERY lane of the wave calls it (a ballot and a DPP
// scan). `head`: the lane's slot lies in the row, is not special and is no continuation; r = the
// slot's own mask_draw at `flat`. Returns whether a span covers the word of the lane's slot. The
// caller must AND the result with !special: a special lane takes the word of the last head below
// it, and before the row's first word that is word = -1, for which this returns true. The state
// between windows is wave-uniform: the words before this window and the furthest reach so far.
__device__ inline bool span_masked(const SpanDraw& S, uint64_t counter, bool head, const uint4& r,
                                   int64_t flat, int32_t& words_before, uint32_t& carry_max) {
  const uint64_t nsh = ballot(head);
  // heads at or below the lane: those below it and its own
  const int32_t word = words_before + (int32_t)popc_below(nsh) + (head ? 1 : 0) - 1;
  uint32_t reach = 0;
  if (head && u01(r.x) < S.p_start) reach = (uint32_t)(word + span_len(S, counter, flat));
  const uint32_t scanned = wave_incl_max(reach);
  const uint32_t best = scanned > carry_max ? scanned : carry_max;
  const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)scanned, 63);
  carry_max = last > carry_max ? last : carry_max;
  words_before += __popcll(nsh);
  return (int32_t)best > word;
}

}  // namespace
}  // namespace lddl
