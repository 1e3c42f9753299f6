// The environment knobs of lddl_tokenize (tokenize_api.hip), read once when a call starts: what
// each accepts and the message it is rejected with, and the word memo's sample size, which two of
// them decide. (Host-only and free of the HIP runtime, like pair_knobs.h, so a CPU program can
// test it: tests/tok_knobs_check.cpp.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "knobs.h"

namespace lddl {

// LDDL_TOKENIZE_PATH (diagnostics, each run by tests/test_tokenize_gpu.py against the oracle):
// "lane" = the fallback kernel for the whole input, "wave" = one sentence per wavefront, "fused" =
// the default, "plain" = the streaming kernel without the word memo.
enum TokPath { kTokFused = 0, kTokPlain, kTokWave, kTokLane };

struct TokKnobs {
  TokPath path = kTokFused;
  // LDDL_TOKENIZE_SLOW, A/B of the streaming kernel's non-ASCII units: "regs" (the default)
  // normalises them from registers (norm_regs), "loop" byte by byte as before
  int32_t slow_loop = 0;
  // LDDL_TOKENIZE_GRID (tests: a smaller grid makes small inputs take the dynamic chunk claims):
  // the most workgroups of a streaming launch, >= 1
  int64_t grid_cap = INT64_MAX;
  // LDDL_TOKENIZE_MEMO_SAMPLE (tests: the memo on small inputs): the sentences of the word
  // memo's sample pass, >= 0; -1: not set (memo_sample)
  int64_t sample = -1;
};

inline int read_tok_knobs(TokKnobs* k) {
  *k = TokKnobs{};
  if (const char* p = getenv("LDDL_TOKENIZE_PATH")) {
    if (!strcmp(p, "lane")) k->path = kTokLane;
    else if (!strcmp(p, "wave")) k->path = kTokWave;
    else if (!strcmp(p, "fused")) k->path = kTokFused;
    else if (!strcmp(p, "plain")) k->path = kTokPlain;
    else LDDL_FAIL(-1, "LDDL_TOKENIZE_PATH must be lane, wave, fused or plain (got %s)", p);
  }
  if (const char* sl = getenv("LDDL_TOKENIZE_SLOW")) {
    if (strcmp(sl, "regs") && strcmp(sl, "loop"))
      LDDL_FAIL(-1, "LDDL_TOKENIZE_SLOW must be regs or loop (got %s)", sl);
    k->slow_loop = !strcmp(sl, "loop");
  }
  int rc;
  if ((rc = read_int_knob("LDDL_TOKENIZE_GRID", 1, "LDDL_TOKENIZE_GRID must be a workgroup count >= 1",
                          &k->grid_cap)) ||
      (rc = read_int_knob("LDDL_TOKENIZE_MEMO_SAMPLE", 0,
                          "LDDL_TOKENIZE_MEMO_SAMPLE must be a sentence count >= 0", &k->sample)))
    return rc;
  return 0;
}

// the word memo's sample (tokenize.hip): 1/32 of the sentences (1/8: 16.06 ms per 2 GB, 1/16:
// 15.68, 1/64: 15.83), at least kMemoMinSample
constexpr int kMemoDiv = 32;
constexpr int64_t kMemoMinSample = 1 << 14;

// The sentences of the leading sample that builds the word memo (the rest reads it), or 0: no
// memo. Off for vocabs whose ids do not fit 16 bits, for inputs too small to repay the second
// launch, and with LDDL_TOKENIZE_PATH=plain; a set LDDL_TOKENIZE_MEMO_SAMPLE is the sample, and
// the memo is on whenever that leaves sentences on both sides.
inline int64_t memo_sample(int64_t n_sent, int32_t vocab_size, const TokKnobs& k) {
  if (vocab_size > 65536 || k.path == kTokPlain) return 0;
  if (k.sample >= 0) return k.sample > 0 && k.sample < n_sent ? k.sample : 0;
  return n_sent >= 4 * kMemoMinSample ? std::max<int64_t>(n_sent / kMemoDiv, kMemoMinSample) : 0;
}

}  // namespace lddl
