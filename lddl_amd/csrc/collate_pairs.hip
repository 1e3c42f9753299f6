// The loader collate straight from a pair table (lddl_pairs_emit's tokens / tok_off / len_a /
// is_rn and, with static masking, pos / labels / pos_off): what collate.hip's encode_kernel
// writes for the strings lddl_render_write makes of the same pairs, without the strings. The ids
// are already ids, so there is nothing to split and no hash to probe: slot x of output row i
// (pair q = rows[i]) is one load,
//     x == 0            [CLS]
//     1 <= x <= na      tokens[tok_off[q] + x - 1]        (A)
//     x == na + 1       [SEP]
//     na + 2 <= x < end - 1   tokens[tok_off[q] + x - 2]  (B)
//     x == end - 1      [SEP]            end = na + nb + 3
//     x >= end          0 (padding)
// which is collate_dev.h's PairSlots over its SlotLayout, shared with pack_kernel like the label
// scatter (scatter_labels); the masking decision of a slot is collate_dev.h's too (MaskDraw,
// mask_draw, mask_apply, word_masked, ContBits), with the same Philox index i * seq_len + x: the
// mask stream is the string kernels' by construction. This unit owns the three row loops and
// their stores; the word loop, one for whole-word and span, writes its two
// predicates out (collate_dev.h says why).
//
//   lddl_collate_pairs          lddl_collate_encode: unmasked (special_tokens_mask) or static
//                               (labels scattered from pos / labels through one LDS row per wave,
//                               so that labels too are written once, coalesced)
//   lddl_collate_pairs_masked   lddl_collate_encode_masked / _masked_ww (no LDS at all)
//   lddl_collate_pairs_masked_span   lddl_collate_encode_masked_span (no LDS)
//
// One wave per output row, kEncWaves rows per block; all offsets 64-bit (a table holds more than
// 2^31 tokens); both id widths of lddl_ctx_id_bytes().
#include "collate_host.h"  // need_vocab, need_static_triple, launch_rows; collate_dev.h
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

struct PairsArgs {
  PairTable P;
  int32_t B, L;
  int32_t cls, sep;
  int64_t* input_ids;
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* special_tokens_mask;  // kPlain without static masking
  int64_t* labels;               // kPlain with static masking, kFused, kFusedWw
  int64_t* nsl;                  // [B]
  int64_t ignore_index;
  MaskDraw draw;
  ContBits cont;
  SpanDraw span;  // kFusedSpan (last: the other modes read their arguments where they were)
};

template <typename ID, int MODE>
__global__ void __launch_bounds__(64 * kEncWaves) pairs_kernel(PairsArgs E) {
  extern __shared__ __attribute__((aligned(16))) int32_t srow[];  // static masking: [waves][L]
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int32_t b = blockIdx.x * kEncWaves + w;
  if (b >= E.B) return;  // the whole wave; no block-wide barrier below
  const int64_t q = E.P.rows ? E.P.rows[b] : (int64_t)b;
  const int64_t t0 = E.P.tok_off[q];
  const int32_t na = E.P.len_a[q];
  const int32_t nb = (int32_t)(E.P.tok_off[q + 1] - t0) - na;
  const int32_t end = na + nb + 3;
  const SlotLayout lay{na, end};
  const int64_t row = (int64_t)b * E.L;
  if (lane == 0) E.nsl[b] = E.P.is_rn[q] ? 1 : 0;

  const PairSlots<ID> slot_id{E.P, t0, lay, E.cls, E.sep};  // the id before masking (x < L)

  if constexpr (MODE == kFusedWw || MODE == kFusedSpan) {
    // windows of 64 slots up to a multiple of 64, the tail predicated: every lane reaches the
    // ballots (and with kFusedSpan the scan) of the word-unit step
    bool carry = false;        // kFusedWw: the state of word_masked between the row's windows
    int32_t words_before = 0;  // kFusedSpan: that of span_masked
    uint32_t carry_max = 0;
    for (int32_t x0 = 0; x0 < E.L; x0 += 64) {
      const int32_t x = x0 + lane;
      const bool in = x < E.L;
      const bool special = x == 0 || x == na + 1 || x >= end - 1;
      const bool prev_special = x <= 1 || x - 1 == na + 1 || x - 1 >= end - 1;  // of slot x - 1
      const int32_t id = in ? slot_id(x) : 0;
      const bool cont = in && !special && !prev_special && cont_id(E.cont, id);
      const uint4 r = mask_draw(E.draw, row + x);
      bool m;  // the one line in which the two word modes differ
      if constexpr (MODE == kFusedSpan)
        m = span_masked(E.span, E.draw.counter, in && !special && !cont, r, row + x,
                        words_before, carry_max);
      else
        m = word_masked(!cont, u01(r.x) < E.draw.p, lane, carry);
      if (in) {
        int64_t lab;
        E.input_ids[row + x] = mask_apply(E.draw, r, !special && m, id, &lab);
        E.labels[row + x] = lab;
        E.token_type_ids[row + x] = lay.segment(x);
        E.attention_mask[row + x] = lay.real(x) ? 1 : 0;
      }
    }
    return;
  } else if constexpr (MODE == kFused) {
    for (int32_t x = lane; x < E.L; x += 64) {
      const bool special = lay.special(x);
      const uint4 r = mask_draw(E.draw, row + x);
      int64_t lab;
      E.input_ids[row + x] = mask_apply(E.draw, r, !special && u01(r.x) < E.draw.p,
                                        slot_id(x), &lab);
      E.labels[row + x] = lab;
      E.token_type_ids[row + x] = lay.segment(x);
      E.attention_mask[row + x] = lay.real(x) ? 1 : 0;
    }
    return;
  } else {
    int32_t* slab = srow + (size_t)w * E.L;
    // labels[b, positions] = the pair's label ids; a position >= L is dropped
    if (E.P.pos) scatter_labels<ID>(E.P, q, slab, E.L, lane);
    for (int32_t x = lane; x < E.L; x += 64) {
      E.input_ids[row + x] = slot_id(x);
      E.token_type_ids[row + x] = lay.segment(x);
      E.attention_mask[row + x] = lay.real(x) ? 1 : 0;
      if (E.P.pos) E.labels[row + x] = slab[x] < 0 ? E.ignore_index : (int64_t)slab[x];
      else E.special_tokens_mask[row + x] = lay.special(x) ? 1 : 0;
    }
  }
}

template <int MODE>
int launch(lddl_ctx* c, const PairsArgs& E, void* stream) {
  const int words = (MODE == kPlain && E.P.pos) ? 1 : 0;
  return c->id_bytes() == 2 ? launch_rows(pairs_kernel<uint16_t, MODE>, E, E.B, words, E.L, stream)
                            : launch_rows(pairs_kernel<int32_t, MODE>, E, E.B, words, E.L, stream);
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_collate_pairs(lddl_ctx* c, void* stream, const void* d_tokens,
                                  const int64_t* d_tok_off, const int32_t* d_len_a,
                                  const uint8_t* d_is_rn, const uint16_t* d_pos, const void* d_lab,
                                  const int64_t* d_pos_off, const int64_t* d_rows, int32_t batch,
                                  int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids,
                                  int64_t* d_attention_mask, int64_t* d_special_tokens_mask,
                                  int64_t* d_labels, int64_t* d_next_sentence_labels,
                                  int64_t ignore_index) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (batch <= 0 || seq_len <= 0) return 0;
  if (need_vocab(c, false)) return -1;
  if (!d_tokens || !d_tok_off || !d_len_a || !d_is_rn) LDDL_FAIL(-1, "null pair table");
  const bool is_static = d_pos != nullptr;
  if (need_static_triple(d_pos, d_lab, d_pos_off)) return -1;
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_next_sentence_labels ||
      (is_static ? !d_labels : !d_special_tokens_mask))
    LDDL_FAIL(-1, "null output");
  PairsArgs E{{d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off, d_rows}, batch,
              seq_len, c->tab.special_id[kCls], c->tab.special_id[kSep], d_input_ids,
              d_token_type_ids, d_attention_mask, d_special_tokens_mask, d_labels,
              d_next_sentence_labels, ignore_index, {}, {}, {}};
  return launch<kPlain>(c, E, stream);
}

// lddl_collate_pairs_masked and, with the span arguments (already validated),
// lddl_collate_pairs_masked_span
static int pairs_masked(lddl_ctx* c, void* stream, const void* d_tokens, const int64_t* d_tok_off,
                        const int32_t* d_len_a, const uint8_t* d_is_rn, const int64_t* d_rows,
                        int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                        int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
                        int64_t* d_next_sentence_labels, float mlm_probability,
                        int64_t ignore_index, int64_t vocab_len, uint64_t seed, uint64_t counter,
                        bool whole_word, const SpanDraw* span) {
  if (batch <= 0 || seq_len <= 0) return 0;
  if (need_vocab(c, true)) return -1;
  if (!d_tokens || !d_tok_off || !d_len_a || !d_is_rn) LDDL_FAIL(-1, "null pair table");
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels ||
      !d_next_sentence_labels)
    LDDL_FAIL(-1, "null output");
  PairsArgs E{{d_tokens, d_tok_off, d_len_a, d_is_rn, nullptr, nullptr, nullptr, d_rows}, batch,
              seq_len, c->tab.special_id[kCls], c->tab.special_id[kSep], d_input_ids,
              d_token_type_ids, d_attention_mask, nullptr, d_labels, d_next_sentence_labels,
              ignore_index,
              mask_draw_of(c, mlm_probability, ignore_index, vocab_len, seed, counter),
              cont_bits_of(c), span ? *span : SpanDraw{}};
  switch (fused_mode(whole_word, span)) {
    case kFusedSpan: return launch<kFusedSpan>(c, E, stream);
    case kFusedWw: return launch<kFusedWw>(c, E, stream);
    default: return launch<kFused>(c, E, stream);
  }
}

extern "C" int lddl_collate_pairs_masked(lddl_ctx* c, void* stream, const void* d_tokens,
                                         const int64_t* d_tok_off, const int32_t* d_len_a,
                                         const uint8_t* d_is_rn, const int64_t* d_rows,
                                         int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                                         int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                         int64_t* d_labels, int64_t* d_next_sentence_labels,
                                         float mlm_probability, int64_t ignore_index,
                                         int64_t vocab_len, uint64_t seed, uint64_t counter,
                                         int32_t whole_word) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  return pairs_masked(c, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_rows, batch, seq_len,
                      d_input_ids, d_token_type_ids, d_attention_mask, d_labels,
                      d_next_sentence_labels, mlm_probability, ignore_index, vocab_len, seed,
                      counter, whole_word != 0, nullptr);
}

extern "C" int lddl_collate_pairs_masked_span(
    lddl_ctx* c, void* stream, const void* d_tokens, const int64_t* d_tok_off,
    const int32_t* d_len_a, const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
    int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids, int64_t* d_attention_mask,
    int64_t* d_labels, int64_t* d_next_sentence_labels, float mlm_probability,
    int64_t ignore_index, int64_t vocab_len, uint64_t seed, uint64_t counter,
    const lddl_span_params* params) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  SpanDraw S;
  if (span_draw_of(params, seed, &S)) return -1;
  return pairs_masked(c, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_rows, batch, seq_len,
                      d_input_ids, d_token_type_ids, d_attention_mask, d_labels,
                      d_next_sentence_labels, mlm_probability, ignore_index, vocab_len, seed,
                      counter, true, &S);
}
