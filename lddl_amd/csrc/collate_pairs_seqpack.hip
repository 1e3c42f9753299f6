// The sequence-packed collate straight from a pair table: to collate_seqpack.hip
// what collate_pairs.hip is to collate.hip. Sample i (pair q = rows[i]) owns the flat slots
// [dst[i], dst[i] + fill[i]) of the [R, L] outputs (the plan of lddl_seqpack_plan, or of
// torch/seqpack.py): slot x < len holds what collate_pairs.hip's pairs_kernel puts at [i, x],
//     x == 0            [CLS]
//     1 <= x <= na      tokens[tok_off[q] + x - 1]        (A)
//     x == na + 1       [SEP]
//     na + 2 <= x < len - 1   tokens[tok_off[q] + x - 2]  (B)
//     x == len - 1      [SEP]            len = na + nb + 3
// plus position_ids = x and sequence_ids = seq_in_row[i]; slots [len, fill) are the row's tail:
// 0 everywhere, labels ignore_index, special_tokens_mask 1. The slot's id, the layout and the
// label scatter are collate_dev.h's (PairSlots, SlotLayout, scatter_labels), shared with
// pairs_kernel; this unit owns the plan's prologue, the predicated window loop and its stores,
// the loop's word branch once for whole-word and span.
// The segments tile the outputs, so
// every element is written once and nothing is cleared beforehand. The per-sample outputs
// (next_sentence_labels, cls_positions, seq_lens) are written by the sample's wave at
// packed_idx[i], its place in (row, start) order.
//
// The Philox index of slot x of sample i is i * draw_stride + x, whole-word windows are 64 slots
// from the sample's start with the carry reset per sample: the masking is that of the unpacked
// batch (lddl_collate_pairs_masked with seq_len = draw_stride), whatever the layout.
//
//   lddl_collate_pairs_seqpack         unmasked (special_tokens_mask) or static (labels through
//                                      one LDS slab of len words per wave)
//   lddl_collate_pairs_seqpack_masked  fused dynamic masking, per token or whole-word (no LDS)
//   lddl_collate_pairs_seqpack_masked_span  fused n-gram (span) masking (no LDS)
//
// One wave per sample, kEncWaves per block; all offsets 64-bit; both id widths of
// lddl_ctx_id_bytes().
#include "collate_host.h"  // need_vocab, need_static_triple, launch_rows; collate_dev.h
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

struct PackArgs {
  PairTable P;
  // the plan, [B] each
  const int64_t* dst;
  const int32_t* fill;
  const int32_t* seq_in_row;
  const int32_t* packed_idx;
  int32_t B, R, L;  // samples, output rows, slots per row
  int32_t draw_stride;
  int32_t cls, sep;
  int64_t* input_ids;
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* special_tokens_mask;  // kPlain without static masking
  int64_t* labels;               // kPlain with static masking, kFused, kFusedWw
  int64_t* position_ids;
  int64_t* sequence_ids;
  int64_t* nsl;            // [B], packed order
  int64_t* cls_positions;  // [B]
  int32_t* seq_lens;       // [B]
  int64_t ignore_index;
  MaskDraw draw;
  ContBits cont;
  SpanDraw span;  // kFusedSpan (last: the other modes read their arguments where they were)
};

template <typename ID, int MODE>
__global__ void __launch_bounds__(64 * kEncWaves) pack_kernel(PackArgs E) {
  extern __shared__ __attribute__((aligned(16))) int32_t srow[];  // static masking: [waves][L]
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int32_t b = blockIdx.x * kEncWaves + w;
  if (b >= E.B) return;  // the whole wave; no block-wide barrier below
  // every load of the prologue is issued before the first wait: the plan's four words beside
  // rows[b], the table's beside each other (two round trips, as in pairs_kernel)
  const int64_t q = E.P.rows ? E.P.rows[b] : (int64_t)b;
  const int64_t o = E.dst[b];
  const int32_t fill = E.fill[b];
  const int32_t at = E.packed_idx[b];
  const int64_t seq = E.seq_in_row[b];
  const int64_t t0 = E.P.tok_off[q];
  const int32_t na = E.P.len_a[q];
  const int32_t nb = (int32_t)(E.P.tok_off[q + 1] - t0) - na;
  const bool rn = E.P.is_rn[q] != 0;
  const int32_t end = na + nb + 3;
  // a sample that takes no row (dst = -1: longer than a row, refused on the host) and a plan
  // that is not this batch's write nothing: no slot outside the outputs is ever touched. One
  // branch ('|', not '||': a chain of exits would wait for each load in turn), which also
  // needs len_a and seq_in_row, so that their loads are not left for after it
  if ((o < 0) | (na < 0) | (nb < 0) | (end > E.L) | (fill < end) |
      (o + fill > (int64_t)E.R * E.L) | (at < 0) | (at >= E.B) | (seq < 1))
    return;
  const int64_t flat = (int64_t)b * E.draw_stride;
  const SlotLayout lay{na, end};
  const PairSlots<ID> slot_id{E.P, t0, lay, E.cls, E.sep};  // the id before masking (x < fill)

  int32_t* slab = srow + (size_t)w * E.L;
  // positions count from the sample's [CLS]; one at or past its end would land in the next
  // sample (refused on the host, dropped here)
  if (MODE == kPlain && E.P.pos) scatter_labels<ID>(E.P, q, slab, end, lane);

  // 64-slot windows from the sample's start, the tail predicated: in the two word modes every
  // lane reaches the ballots (and with kFusedSpan the scan) of the word-unit step
  bool carry = false;        // kFusedWw: the state of word_masked, per sample
  int32_t words_before = 0;  // kFusedSpan: that of span_masked, per sample like carry
  uint32_t carry_max = 0;
  for (int32_t x0 = 0; x0 < fill; x0 += 64) {
    const int32_t x = x0 + lane;
    const bool in = x < fill, real = x < end;
    const bool special = lay.special(x);
    const int32_t id = in ? slot_id(x) : 0;
    int64_t out = id, lab = E.ignore_index;
    if constexpr (MODE == kFusedWw || MODE == kFusedSpan) {
      const bool prev_special = x <= 1 || x - 1 == na + 1 || x - 1 >= end - 1;  // of slot x - 1
      const bool cont = in && !special && !prev_special && cont_id(E.cont, id);
      const uint4 r = mask_draw(E.draw, flat + x);
      bool m;  // the one line in which the two word modes differ
      if constexpr (MODE == kFusedSpan)
        m = span_masked(E.span, E.draw.counter, in && !special && !cont, r, flat + x,
                        words_before, carry_max);
      else
        m = word_masked(!cont, u01(r.x) < E.draw.p, lane, carry);
      out = mask_apply(E.draw, r, !special && m, id, &lab);
    } else if constexpr (MODE == kFused) {
      if (real) out = mask_slot(E.draw, flat + x, special, id, &lab);
    } else {
      if (E.P.pos && real && slab[x] >= 0) lab = slab[x];
    }
    if (in) {
      E.input_ids[o + x] = out;
      E.token_type_ids[o + x] = (x >= na + 2 && real) ? 1 : 0;
      E.attention_mask[o + x] = real ? 1 : 0;
      E.position_ids[o + x] = real ? x : 0;
      E.sequence_ids[o + x] = real ? seq : 0;
      if (MODE != kPlain || E.P.pos) E.labels[o + x] = lab;
      else E.special_tokens_mask[o + x] = special ? 1 : 0;
    }
  }
  if (lane == 0) {  // last: is_rn's load has the window loop to arrive in
    E.nsl[at] = rn ? 1 : 0;
    E.cls_positions[at] = o;
    E.seq_lens[at] = end;
  }
}

template <int MODE>
int launch(lddl_ctx* c, const PackArgs& E, void* stream) {
  const int words = (MODE == kPlain && E.P.pos) ? 1 : 0;
  return c->id_bytes() == 2 ? launch_rows(pack_kernel<uint16_t, MODE>, E, E.B, words, E.L, stream)
                            : launch_rows(pack_kernel<int32_t, MODE>, E, E.B, words, E.L, stream);
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_collate_pairs_seqpack(
    lddl_ctx* c, void* stream, const void* d_tokens, const int64_t* d_tok_off,
    const int32_t* d_len_a, const uint8_t* d_is_rn, const uint16_t* d_pos, const void* d_lab,
    const int64_t* d_pos_off, const int64_t* d_rows, int32_t batch, const int64_t* d_dst,
    const int32_t* d_fill, const int32_t* d_seq_in_row, const int32_t* d_packed_idx,
    int32_t out_rows, int32_t max_seq_length, int64_t* d_input_ids, int64_t* d_token_type_ids,
    int64_t* d_attention_mask, int64_t* d_special_tokens_mask, int64_t* d_labels,
    int64_t* d_position_ids, int64_t* d_sequence_ids, int64_t* d_next_sentence_labels,
    int64_t* d_cls_positions, int32_t* d_seq_lens, int64_t ignore_index) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (batch <= 0 || out_rows <= 0 || max_seq_length <= 0) return 0;
  if (need_vocab(c, false)) return -1;
  if (!d_tokens || !d_tok_off || !d_len_a || !d_is_rn) LDDL_FAIL(-1, "null pair table");
  if (!d_dst || !d_fill || !d_seq_in_row || !d_packed_idx) LDDL_FAIL(-1, "null plan");
  const bool is_static = d_pos != nullptr;
  if (need_static_triple(d_pos, d_lab, d_pos_off)) return -1;
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_position_ids ||
      !d_sequence_ids || !d_next_sentence_labels || !d_cls_positions || !d_seq_lens ||
      (is_static ? !d_labels : !d_special_tokens_mask))
    LDDL_FAIL(-1, "null output");
  PackArgs E{{d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off, d_rows}, d_dst,
             d_fill, d_seq_in_row, d_packed_idx, batch, out_rows, max_seq_length, 0,
             c->tab.special_id[kCls], c->tab.special_id[kSep], d_input_ids, d_token_type_ids,
             d_attention_mask, d_special_tokens_mask, d_labels, d_position_ids, d_sequence_ids,
             d_next_sentence_labels, d_cls_positions, d_seq_lens, ignore_index, {}, {}, {}};
  return launch<kPlain>(c, E, stream);
}

// lddl_collate_pairs_seqpack_masked and, with the span arguments (already validated),
// lddl_collate_pairs_seqpack_masked_span
static int pairs_seqpack_masked(lddl_ctx* c, void* stream, const void* d_tokens,
                                const int64_t* d_tok_off, const int32_t* d_len_a,
                                const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
                                const int64_t* d_dst, const int32_t* d_fill,
                                const int32_t* d_seq_in_row, const int32_t* d_packed_idx,
                                int32_t out_rows, int32_t max_seq_length, int32_t draw_stride,
                                int64_t* d_input_ids, int64_t* d_token_type_ids,
                                int64_t* d_attention_mask, int64_t* d_labels,
                                int64_t* d_position_ids, int64_t* d_sequence_ids,
                                int64_t* d_next_sentence_labels, int64_t* d_cls_positions,
                                int32_t* d_seq_lens, float mlm_probability, int64_t ignore_index,
                                int64_t vocab_len, uint64_t seed, uint64_t counter,
                                bool whole_word, const SpanDraw* span) {
  if (batch <= 0 || out_rows <= 0 || max_seq_length <= 0) return 0;
  if (need_vocab(c, true)) return -1;
  if (!d_tokens || !d_tok_off || !d_len_a || !d_is_rn) LDDL_FAIL(-1, "null pair table");
  if (!d_dst || !d_fill || !d_seq_in_row || !d_packed_idx) LDDL_FAIL(-1, "null plan");
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels || !d_position_ids ||
      !d_sequence_ids || !d_next_sentence_labels || !d_cls_positions || !d_seq_lens)
    LDDL_FAIL(-1, "null output");
  PackArgs E{{d_tokens, d_tok_off, d_len_a, d_is_rn, nullptr, nullptr, nullptr, d_rows}, d_dst,
             d_fill, d_seq_in_row, d_packed_idx, batch, out_rows, max_seq_length, draw_stride,
             c->tab.special_id[kCls], c->tab.special_id[kSep], d_input_ids, d_token_type_ids,
             d_attention_mask, nullptr, d_labels, d_position_ids, d_sequence_ids,
             d_next_sentence_labels, d_cls_positions, d_seq_lens, ignore_index,
             mask_draw_of(c, mlm_probability, ignore_index, vocab_len, seed, counter),
             cont_bits_of(c), span ? *span : SpanDraw{}};
  switch (fused_mode(whole_word, span)) {
    case kFusedSpan: return launch<kFusedSpan>(c, E, stream);
    case kFusedWw: return launch<kFusedWw>(c, E, stream);
    default: return launch<kFused>(c, E, stream);
  }
}

extern "C" int lddl_collate_pairs_seqpack_masked(
    lddl_ctx* c, void* stream, const void* d_tokens, const int64_t* d_tok_off,
    const int32_t* d_len_a, const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
    const int64_t* d_dst, const int32_t* d_fill, const int32_t* d_seq_in_row,
    const int32_t* d_packed_idx, int32_t out_rows, int32_t max_seq_length, int32_t draw_stride,
    int64_t* d_input_ids, int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
    int64_t* d_position_ids, int64_t* d_sequence_ids, int64_t* d_next_sentence_labels,
    int64_t* d_cls_positions, int32_t* d_seq_lens, float mlm_probability, int64_t ignore_index,
    int64_t vocab_len, uint64_t seed, uint64_t counter, int32_t whole_word) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  return pairs_seqpack_masked(c, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_rows, batch,
                              d_dst, d_fill, d_seq_in_row, d_packed_idx, out_rows, max_seq_length,
                              draw_stride, d_input_ids, d_token_type_ids, d_attention_mask,
                              d_labels, d_position_ids, d_sequence_ids, d_next_sentence_labels,
                              d_cls_positions, d_seq_lens, mlm_probability, ignore_index, vocab_len,
                              seed, counter, whole_word != 0, nullptr);
}

extern "C" int lddl_collate_pairs_seqpack_masked_span(
    lddl_ctx* c, void* stream, const void* d_tokens, const int64_t* d_tok_off,
    const int32_t* d_len_a, const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
    const int64_t* d_dst, const int32_t* d_fill, const int32_t* d_seq_in_row,
    const int32_t* d_packed_idx, int32_t out_rows, int32_t max_seq_length, int32_t draw_stride,
    int64_t* d_input_ids, int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
    int64_t* d_position_ids, int64_t* d_sequence_ids, int64_t* d_next_sentence_labels,
    int64_t* d_cls_positions, int32_t* d_seq_lens, float mlm_probability, int64_t ignore_index,
    int64_t vocab_len, uint64_t seed, uint64_t counter, const lddl_span_params* params) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  SpanDraw S;
  if (span_draw_of(params, seed, &S)) return -1;
  return pairs_seqpack_masked(c, stream, d_tokens, d_tok_off, d_len_a, d_is_rn, d_rows, batch,
                              d_dst, d_fill, d_seq_in_row, d_packed_idx, out_rows, max_seq_length,
                              draw_stride, d_input_ids, d_token_type_ids, d_attention_mask,
                              d_labels, d_position_ids, d_sequence_ids, d_next_sentence_labels,
                              d_cls_positions, d_seq_lens, mlm_probability, ignore_index, vocab_len,
                              seed, counter, true, &S);
}
