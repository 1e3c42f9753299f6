// Tokenizer, the entry point (unit map: tokenize.hip): lddl_tokenize checks its arguments, reads
// the knobs, takes the fallback list, and runs the path the knobs choose through the launchers
// of the kernels' units (tokenize_plan.h). It launches no kernel itself.
#include "tokenize_plan.h"

using namespace lddl;

extern "C" int lddl_tokenize(lddl_ctx* c, void* stream, const uint8_t* d_text, int64_t n_bytes,
                             const int64_t* d_sent_off, int64_t n_sent, int32_t max_pieces,
                             int32_t* d_ids, int32_t* d_sent_len) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (n_sent < 0 || n_bytes < 0 || max_pieces <= 0 || max_pieces > (1 << 24))
    LDDL_FAIL(-1, "bad sizes (max_pieces must be in 1 .. 2^24)");
  if (n_sent >= (int64_t)INT32_MAX - (1 << 22)) LDDL_FAIL(-1, "too many sentences in one call (%lld)", (long long)n_sent);
  if (n_sent == 0) return 0;
  // (Round 6's split form — phase B and placement in launches of their own — measured slower and
  // lives on branch ab/tok-split)
  hipStream_t st = as_stream(stream);
  TokCall T{c, st, d_text, n_bytes, d_sent_off, n_sent, max_pieces, d_ids, d_sent_len};
  const TokKnobs& knobs = T.knobs;
  int rc;
  if ((rc = read_tok_knobs(&T.knobs))) return rc;
  if (knobs.path == kTokLane) return launch_lane(T, 0, n_sent, 65536, true);
  ArenaTmp fbb(&c->arena, st);
  LDDL_HIP(fbb.take(sizeof(int32_t) * (size_t)(n_sent + kFbHead + 1)));
  T.fb = fbb.as<int32_t>();
  T.chunk_ctr = T.fb + kFbHead + n_sent;
  LDDL_HIP(hipMemsetAsync(T.fb, 0, sizeof(int32_t) * kFbHead, st));
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  T.n_cu = n_cu;
  if (knobs.path == kTokWave) return tokenize_wave(T);
  int64_t grid_max;
  if ((rc = batch_grid_max(T, &grid_max))) return rc;
#ifdef LDDL_STAMPS
  ArenaScope diag(&c->arena, st);
  unsigned long long *tl, *rg;
  if ((rc = stamps_begin(diag, T, grid_max, &tl, &rg))) return rc;
#endif
  // the word memo (tokenize.hip): a leading sample of the sentences builds it, the rest reads it
  const int64_t n_sample = memo_sample(n_sent, c->vocab_size, knobs);
  if (!n_sample) {
    if ((rc = batch_pass(T, grid_max, 0, n_sent, kMemoOff, WordMemo{nullptr, 0}))) return rc;
  } else {
    ArenaTmp mb(&c->arena, st);
    const size_t entries = (size_t)1 << kMemoLog2;
    LDDL_HIP(mb.take(64 * entries));
    LDDL_HIP(hipMemsetAsync(mb.as<void>(), 0, 64 * entries, st));
    const WordMemo M{mb.as<uint4>(), (uint32_t)(entries - 1)};
    if ((rc = batch_pass(T, grid_max, 0, n_sample, kMemoBuild, M)) ||
        (rc = batch_pass(T, grid_max, n_sample, n_sent - n_sample, kMemoLookup, M)))
      return rc;
  }
#ifdef LDDL_STAMPS
  if ((rc = report_tok_stamps(T, tl, rg))) return rc;
#endif
  return 0;
}
