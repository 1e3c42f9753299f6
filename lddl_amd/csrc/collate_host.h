// Host helpers shared by the entry points of the collate units (collate.hip,
// collate_seqpack.hip, collate_pairs.hip, collate_pairs_seqpack.hip): the refusals they have in
// common, the masking arguments from the context, the span arguments from the caller's struct
// and the one launch of a kernel with kEncWaves samples per block. Each translation unit gets
// its own copy (anonymous namespace).
#pragma once
#include "collate_dev.h"
#include "lddl_amd.h"
#include "span_dev.h"

namespace lddl {
namespace {

// the special ids a collate writes: [CLS] and [SEP], and [MASK] with fused dynamic masking
inline int need_vocab(const lddl_ctx* c, bool mask) {
  const bool ok = c->tab.special_id[kCls] >= 0 && c->tab.special_id[kSep] >= 0;
  if (mask) {
    if (!ok || c->tab.special_id[kMask] < 0) LDDL_FAIL(-1, "vocab needs [CLS], [SEP] and [MASK]");
  } else if (!ok) {
    LDDL_FAIL(-1, "vocab needs [CLS] and [SEP]");
  }
  return 0;
}

// a pair table's static masking comes as pos, labels and pos_off
inline int need_static_triple(const void* pos, const void* lab, const void* pos_off) {
  if ((lab != nullptr) != (pos != nullptr) || (pos_off != nullptr) != (pos != nullptr))
    LDDL_FAIL(-1, "static masking needs pos, labels and pos_off, all three or none");
  return 0;
}

inline MaskDraw mask_draw_of(const lddl_ctx* c, float p, int64_t ignore_index, int64_t vocab_len,
                             uint64_t seed, uint64_t counter) {
  return MaskDraw{p, ignore_index, c->tab.special_id[kMask], vocab_len, seed, counter};
}
inline ContBits cont_bits_of(const lddl_ctx* c) { return ContBits{c->d_cont_bits, c->vocab_size}; }

// The span arguments of a kernel from the caller's lddl_span_params (lddl_span_params_make's
// output): refused unless it is one that function can have written.
inline int span_draw_of(const lddl_span_params* sp, uint64_t seed, SpanDraw* out) {
  if (!sp) LDDL_FAIL(-1, "null span params");
  bool ok = sp->n >= 1 && sp->n <= kSpanMaxN && sp->p_start >= 0.f && sp->p_start <= 1.f;
  float prev = 0.f;
  for (int k = 0; ok && k < kSpanMaxN - 1; ++k) {
    const float c = sp->cum[k];
    ok = k < sp->n - 1 ? (c >= prev && c <= 1.f) : c == 1.f;
    prev = c;
  }
  if (!ok) LDDL_FAIL(-1, "invalid span params (not made by lddl_span_params_make)");
  out->p_start = sp->p_start;
  out->seed2 = seed ^ LDDL_SPAN_SEED_XOR;
  for (int k = 0; k < kSpanMaxN - 1; ++k) out->cum[k] = sp->cum[k];
  return 0;
}

// the MODE of a fused-masking entry point: the span arguments given, else the whole-word flag
inline int fused_mode(bool whole_word, const SpanDraw* span) {
  return span ? kFusedSpan : whole_word ? kFusedWw : kFused;
}

// One wave per sample, kEncWaves samples per block, `words` int32 of LDS per slot and wave.
template <typename Args>
int launch_rows(void (*kernel)(Args), const Args& args, int32_t B, int words, int32_t L,
                void* stream) {
  const size_t lds = sizeof(int32_t) * (size_t)words * (size_t)L * kEncWaves;
  if (lds > 160 * 1024) LDDL_FAIL(-1, "sequence length %d too long for the collate kernel", L);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((B + kEncWaves - 1) / kEncWaves)),
                     dim3(64 * kEncWaves), lds, as_stream(stream), args);
  LDDL_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace lddl
