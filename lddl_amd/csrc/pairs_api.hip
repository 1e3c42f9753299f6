// NSP pair construction + static MLM masking on the GPU: the orchestration of the pair stage. This
// file checks the arguments and knobs, runs the stages in order and holds the C entry points; it
// launches no kernel of its own. Each stage's kernels and the host function that launches them
// are one unit:
//   pairs_plan.h       the records the stages share, the plan's state, the stage functions
//   pair_knobs.h       every environment knob of a plan, read when it starts (host-only)
//   plan_split.h       the replay plan's host decisions: its mode, the split point, the ring
//   pairs_compact.hip  compaction of the tokenizer's output (compact_inputs)
//   pairs.hip          the replay planner: plan_replay_kernel and its three small kernels; the plan's
//                      mode, an attempt's pools and a range's read-back (it keeps the file, and
//                      with it the history of the code most changes touch)
//   replay_rng.h       its device pieces: CPython's MT19937 wave-uniform (WaveRng),
//   replay_len.h         the sentence-length window (LenWin, span_token),
//   replay_slice.h       the time-sliced queue: protocol, save area, claim and publish, kPlanLds
//   densify_dev.h      one wave's share of the dense packing (the planner's dense workgroups too)
//   pairs_densify.hip  the dense packing as launches of its own (launch_densify, launch_densify_head)
//   pairs_native.hip   the native planner: the walk, the keyed order, plan_native
//   pairs_native_mask.hip  its two mask kernels, plain and whole-word (launch_native_masks)
//   native_dev.h       what the two share on the device: the Philox streams, NativeArgs
//   native_shape.h     the native launches' LDS sizes, grids and blocks (host-only)
//   pairs_shuffle.hip  the replay plan's partition shuffle (shuffle_partitions)
//   pairs_layout.hip   gather records, output-order scans, mask replay (layout_*)
//   pairs_gather.hip   the gather (emit_ranges)
//
// Reference: lddl/dask/bert/pretrain.py
//   _get_documents filtering       89-97   -> scatter_sentences_kernel, scatter_docs_kernel,
//                                             part_offsets_kernel (drop empty sentences / documents)
//   _to_partition_pairs           386-402  -> plan_replay_kernel / plan_native_kernel (a wave /
//                                             a workgroup per partition) + the partition shuffle
//                                             (shuffle_sort_kernel; native: order_native_kernel)
//   create_pairs_from_document    241-365  -> the document loop of plan_replay_kernel /
//                                             plan_native_kernel
//   _truncate_seq_pair            161-176  -> WaveRng::trunc_draws / its closed form in
//                                             plan_native_kernel
//   create_masked_lm_predictions  182-238  -> decisions: WaveRng::mask_decisions, mask_native_kernel;
//                                             positions: fy_resolve_kernel; applied by the gather
//
// Split into a control plane that touches only integers (sentence lengths, RNG draws) and a data
// plane that moves tokens:
//   plan    one wave per partition. Replay mode reproduces CPython's `random` exactly
//           (random.seed(part_seed[p]) then the reference's draw sequence): the wave executes the
//           sequential algorithm wave-uniformly (every lane computes the same scalars, so control
//           flow never diverges), keeps the MT19937 state in LDS and regenerates it with a
//           64-lane cooperative twist. Output: 32-byte pair descriptors (sentence span + truncation
//           window of A and B) and, with masking, the chosen positions + replacement ids.
//   layout  scans of per-partition pair counts and per-pair token / mask counts (final order =
//           the partition shuffle of pretrain.py:401).
//   gather  one wave per pair: coalesced copy of A and B token spans from the tokenizer output,
//           applying the mask decisions and emitting positions + labels.
#include "pairs_plan.h"

using namespace lddl;

// static masking: the gather keeps a decision per token of the sequence in LDS (pairs_gather.hip)
constexpr int kMaxSeqGather = 4096;

static int check_plan_args(const lddl_ctx* c, const lddl_pair_params* prm, PlanKnobs* knobs) {
  if (!c || !prm) LDDL_FAIL(-1, "null argument");
  if (prm->seq < 5 || prm->seq > 65535) LDDL_FAIL(-1, "target_seq_length %d out of range", prm->seq);
  if (prm->dup < 1) LDDL_FAIL(-1, "duplicate_factor must be >= 1");
  if (prm->rng != LDDL_RNG_REPLAY && prm->rng != LDDL_RNG_NATIVE)
    LDDL_FAIL(-1, "unknown rng mode %d", prm->rng);
  if (prm->masking && prm->seq > kMaxSeqGather)
    LDDL_FAIL(-1, "static masking supports target_seq_length <= %d", kMaxSeqGather);
  if (prm->masking && (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0 ||
                       c->tab.special_id[kMask] < 0))
    LDDL_FAIL(-1, "static masking needs [CLS] [SEP] [MASK] in the vocab");
  if (prm->whole_word && !prm->masking) LDDL_FAIL(-1, "whole_word needs static masking (masking = 1)");
  if (prm->whole_word && prm->rng != LDDL_RNG_NATIVE)
    LDDL_FAIL(-1, "whole_word needs rng = LDDL_RNG_NATIVE (the replay mode reproduces the "
                  "reference, which has no whole-word masking)");
  return read_plan_knobs(knobs);
}

// Everything downstream of the planner for a one-range replay plan. Without masking, pair_prep
// builds the records from the output order.
static int finish_unsplit(lddl_pairs* P, PlanWork& W) {
  int rc;
  P->n_rg = 1;
  PairRange& r = P->rg[0];
  r = PairRange{};
  r.p1 = W.n_part;
  r.n_pairs = P->n_pairs;
  if ((rc = shuffle_partitions(P, W, r, P->part_base))) return rc;
#ifdef LDDL_STAMPS
  if ((rc = report_plan_stamps(W))) return rc;
#endif
  return P->masking ? layout_replay(P, W, r) : layout_pairs(P, W);
}

static int32_t max_predictions(const lddl_pair_params* prm) {
  if (!prm->masking) return 0;
  const int32_t m = (int32_t)rint((double)prm->seq * prm->masked_lm_ratio);
  return std::min(std::max(m, 1), prm->seq);
}

// First half of a plan: the whole plan when it is not split (native RNG, no masking, too few
// partitions); else the head range planned, resolved and laid out while the tail range's
// planner still runs on the side stream (P->work carries the call over to plan_tail_stage).
static int plan_head_stage(lddl_pairs* P, const int64_t* d_sent_off, const int32_t* d_sent_len,
                           const int64_t* d_doc_sent_off, int64_t n_doc,
                           const int64_t* d_part_doc_off) {
  PlanWork& W = *P->work;
  int rc;
  if ((rc = compact_inputs(P, W, d_sent_off, d_sent_len, d_doc_sent_off, n_doc, d_part_doc_off)))
    return rc;
  if (W.prm->rng == LDDL_RNG_NATIVE) {
    if ((rc = plan_native(P, W))) return rc;
  } else {
    if ((rc = plan_replay_setup(P, W)) || (rc = choose_mode(P, W))) return rc;
    if (!W.split.s) {
      if ((rc = plan_replay_unsplit(P, W, 0)) || (rc = finish_unsplit(P, W))) return rc;
    } else {
      bool usable = false;
      if ((rc = plan_replay_split_head(P, W, &usable))) return rc;
      PairRange& r = P->rg[0];
      if (usable) {
        if ((rc = shuffle_partitions(P, W, r, P->part_base)) || (rc = layout_replay(P, W, r))) return rc;
        P->head_valid = true;
      }
    }
  }
  LDDL_HIP(hipStreamSynchronize(W.st));  // the ranges' totals (layout_scan)
  if (!W.split.s) {
    P->n_tokens = P->rg[0].n_tokens;
    P->n_masked = P->rg[0].n_masked;
    P->work.reset();
  }
  return 0;
}

// Second half of a split plan: joins the tail range, then either lays it out behind the head
// (offsets carried in as the range's bases) or, when a pool overflowed, drops the head's tables
// and plans everything again in one range with the exact pool sizes.
static int plan_tail_stage(lddl_pairs* P) {
  if (!P->work) return 0;
  PlanWork& W = *P->work;
  int rc;
  unsigned long long ctl[4];
  PairRange &h = P->rg[0], &t = P->rg[1];
  if ((rc = plan_replay_split_tail(P, W, ctl))) return rc;
  // the head's shuffle and layout temporaries: the tail range (or the re-plan) takes its own
  for (void* b : {(void*)W.rt.M.slots, (void*)W.rt.M.dstq, (void*)W.rt.pcnt, (void*)W.rt.scr2})
    if (b) W.tmp.give(b);
  W.rt = RangeTmp{};
  if (ctl[1]) {  // a pool overflowed: the head's output is void; one range (h), exact sizes
    P->head_valid = false;
    drop_pools(P, W);
    grow_pools(W, ctl);
    t = PairRange{};
    W.split.s = 0;
    if ((rc = plan_replay_unsplit(P, W, 1)) || (rc = finish_unsplit(P, W))) return rc;
  } else {
    if ((rc = tail_part_base(P, W))) return rc;
    t.p0 = W.split.s;
    t.p1 = W.n_part;
    t.pair0 = h.n_pairs;
    t.tok0 = h.n_tokens;
    t.pos0 = h.n_masked;
    P->n_rg = 2;
    if ((rc = shuffle_partitions(P, W, t, W.split.tail_rel)) || (rc = layout_replay(P, W, t))) return rc;
  }
  LDDL_HIP(hipStreamSynchronize(W.st));
  P->n_pairs = h.n_pairs + t.n_pairs;
  P->n_tokens = h.n_tokens + t.n_tokens;
  P->n_masked = h.n_masked + t.n_masked;
  P->work.reset();
  return 0;
}

static void plan_counts(const lddl_pairs* P, int64_t* counts) {
  if (!counts) return;
  counts[0] = P->n_pairs;
  counts[1] = P->n_tokens;
  counts[2] = P->n_masked;
  counts[3] = P->n_kept_sent;
  counts[4] = P->n_kept_doc;
}

extern "C" int lddl_pairs_plan_head(lddl_ctx* c, void* stream, const lddl_pair_params* prm,
                                    const int64_t* d_sent_off, const int32_t* d_ids,
                                    const int32_t* d_sent_len, int64_t n_sent,
                                    const int64_t* d_doc_sent_off, int64_t n_doc,
                                    const int64_t* d_part_doc_off, const int64_t* d_part_seed,
                                    int64_t n_part, lddl_pairs** out, int64_t* head) {
  if (out) *out = nullptr;
  PlanKnobs knobs;
  int rc;
  if (!out) LDDL_FAIL(-1, "null argument");
  if ((rc = check_plan_args(c, prm, &knobs))) return rc;
  hipStream_t st = as_stream(stream);
  // until it is handed out, an error return drops the plan: its blocks go back on `st` (after
  // the tail launch, when one is in flight)
  std::unique_ptr<lddl_pairs> P(new lddl_pairs(&c->arena, st));
  P->n_part = n_part;
  P->prm = *prm;
  P->masking = prm->masking;
  P->seq = prm->seq;
  P->cls_id = c->tab.special_id[kCls];
  P->sep_id = c->tab.special_id[kSep];
  P->max_pred = max_predictions(prm);
  LDDL_HIP(hipEventCreate(&P->ev[0]));
  LDDL_HIP(hipEventCreate(&P->ev[1]));
  P->work.reset(new PlanWork(c, &P->prm, d_ids, d_part_seed, n_sent, n_part, st, P->mem, knobs));
  if ((rc = plan_head_stage(P.get(), d_sent_off, d_sent_len, d_doc_sent_off, n_doc, d_part_doc_off)))
    return rc;
  if (head) {
    for (int i = 0; i < 8; ++i) head[i] = 0;
    if (P->work) {  // split: the head's counts and what they predict for the whole plan
      const PlanWork& W = *P->work;
      const PairRange& h = P->rg[0];
      head[0] = 1;
      head[1] = h.n_pairs;
      head[2] = h.n_tokens;
      head[3] = h.n_masked;
      for (int i = 4; i < 7; ++i) head[i] = plan_suggest_capacity(head[i - 3], W.n_kept_tok, W.split.h_info[1]);
    }
    head[7] = P->n_slices;
  }
  *out = P.release();
  return 0;
}

extern "C" int lddl_pairs_plan_tail(lddl_pairs* P, int64_t* counts, int32_t* head_valid) {
  if (!P) LDDL_FAIL(-1, "null plan");
  int rc;
  if ((rc = plan_tail_stage(P))) return rc;
  plan_counts(P, counts);
  if (head_valid) *head_valid = P->head_valid ? 1 : 0;
  return 0;
}

extern "C" int lddl_pairs_plan(lddl_ctx* c, void* stream, const lddl_pair_params* prm,
                               const int64_t* d_sent_off, const int32_t* d_ids,
                               const int32_t* d_sent_len, int64_t n_sent,
                               const int64_t* d_doc_sent_off, int64_t n_doc,
                               const int64_t* d_part_doc_off, const int64_t* d_part_seed,
                               int64_t n_part, lddl_pairs** out, int64_t* counts) {
  lddl_pairs* P = nullptr;
  int rc;
  if (out) *out = nullptr;
  if ((rc = lddl_pairs_plan_head(c, stream, prm, d_sent_off, d_ids, d_sent_len, n_sent, d_doc_sent_off,
                                 n_doc, d_part_doc_off, d_part_seed, n_part, &P, nullptr)))
    return rc;
  if ((rc = lddl_pairs_plan_tail(P, counts, nullptr))) {
    delete P;  // (joins, then its blocks go back on the planning stream)
    return rc;
  }
  *out = P;
  return 0;
}

extern "C" int lddl_pairs_emit(lddl_pairs* P, void* stream, void* d_tokens, int64_t* d_tok_off,
                               int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                               int64_t* d_pos_off) {
  if (!P) LDDL_FAIL(-1, "null plan");
  if (P->work) LDDL_FAIL(-1, "lddl_pairs_emit before lddl_pairs_plan_tail");
  return emit_ranges(P, 0, P->n_rg, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab,
                     d_pos_off);
}

extern "C" int lddl_pairs_emit_head(lddl_pairs* P, void* stream, void* d_tokens, int64_t* d_tok_off,
                                    int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                                    int64_t* d_pos_off) {
  if (!P) LDDL_FAIL(-1, "null plan");
  if (!P->work) LDDL_FAIL(-1, "lddl_pairs_emit_head: not a split plan between its head and tail calls");
  if (!P->head_valid) return 0;  // (a pool overflowed: lddl_pairs_plan_tail will say so)
  return emit_ranges(P, 0, 1, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off);
}

extern "C" int lddl_pairs_emit_tail(lddl_pairs* P, void* stream, void* d_tokens, int64_t* d_tok_off,
                                    int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                                    int64_t* d_pos_off) {
  if (!P) LDDL_FAIL(-1, "null plan");
  if (P->work || P->n_rg != 2 || !P->head_valid)
    LDDL_FAIL(-1, "lddl_pairs_emit_tail: no valid head range (use lddl_pairs_emit)");
  return emit_ranges(P, 1, 2, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off);
}

extern "C" int lddl_pairs_destroy(lddl_pairs* P, void* stream) {
  if (!P) return 0;
  P->join(as_stream(stream));  // (a split plan dropped before its tail call)
  P->mem.release(as_stream(stream));  // (the last use of the blocks was on this stream)
  delete P;
  return 0;
}

extern "C" int lddl_pairs_plan_ms(const lddl_pairs* P, float* ms) {
  if (!P || !ms) LDDL_FAIL(-1, "null argument");
  *ms = 0.f;
  if (P->n_part && P->ev[0]) LDDL_HIP(hipEventElapsedTime(ms, P->ev[0], P->ev[1]));
  return 0;
}

extern "C" int lddl_pairs_part_offsets(lddl_pairs* P, void* stream, int64_t* d_part_pair_off) {
  if (!P || !d_part_pair_off) LDDL_FAIL(-1, "null argument");
  LDDL_HIP(hipMemcpyAsync(d_part_pair_off, P->part_base, 8 * (P->n_part + 1),
                          hipMemcpyDeviceToDevice, as_stream(stream)));
  return 0;
}
