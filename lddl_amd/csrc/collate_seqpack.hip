// Sequence-packed collate: the loader's collate with several samples per row.
//
//   lddl_collate_seqpack         lddl_collate_encode into a segment of a shared row: static
//                                masking (labels from masked_lm_positions / masked_lm_labels) or
//                                dynamic unmasked (special_tokens_mask).
//   lddl_collate_seqpack_masked  lddl_collate_encode_masked / _masked_ww likewise.
//   lddl_collate_seqpack_masked_span  lddl_collate_encode_masked_span likewise.
//
// The host plans the rows (torch/seqpack.py): sample i owns the flat slots
// [dst[i], dst[i] + fill[i]) of the [R, L] outputs, its tokens first and, for the last sample of
// a row, the row's unused tail behind them. The segments tile the outputs, so every element is
// written exactly once and nothing is cleared beforehand. One wave per sample, the segment
// staged in LDS as in encode_kernel, whose string-side arguments it shares (collate_dev.h's
// StrSample, StrLabels); the staging and the window loop are written out here, as the comment
// at collate_dev.h's SlotLayout explains, the loop's word branch once for whole-word and span
// (DESIGN §26). The Philox index of slot x of sample i is
// i * draw_stride + x: the masking is that of the unpacked batch, whatever the layout.
#include "collate_host.h"  // need_vocab, launch_rows; collate_dev.h
#include "lddl_amd.h"

namespace lddl {
namespace {

struct SeqpackArgs {
  StrSample S;
  const int64_t* dst;         // [B] flat slot row * L + start of the sample's [CLS]
  const int32_t* fill;        // [B] slots the sample's wave writes (>= na + nb + 3)
  const int32_t* seq_in_row;  // [B] 1-based
  int32_t B, L;
  int64_t* input_ids;
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* position_ids;
  int64_t* sequence_ids;
  int64_t* labels;               // static or fused masking, else null
  int64_t* special_tokens_mask;  // dynamic unmasked, else null
  StrLabels G;
  int64_t ignore_index;
  int32_t draw_stride;
  MaskDraw draw;
  ContBits cont;
  SpanDraw span;  // kFusedSpan (last: the other modes read their arguments where they were)
};

template <int MODE>
__global__ void __launch_bounds__(64 * kEncWaves) seqpack_kernel(SeqpackArgs E) {
  extern __shared__ __attribute__((aligned(16))) int32_t srow[];
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int b = blockIdx.x * kEncWaves + w;
  const int32_t na = b < E.B ? E.S.na[b] : 0, nb = b < E.B ? E.S.nb[b] : 0;
  const int32_t end = na + nb + 3;
  // a sample that does not fit its row is refused on the host; here it must not leave the LDS
  const bool active = b < E.B && end <= E.L;
  const int32_t fill = active ? min(E.fill[b], E.L) : 0;
  int32_t* sid = srow + (size_t)w * 2 * E.L;
  int32_t* slab = sid + E.L;
  const int32_t cls = E.S.T.special_id[kCls], sep = E.S.T.special_id[kSep];
  for (int32_t x = lane; x < fill; x += 64) {
    if (x == 0) sid[x] = cls;
    else if (x == na + 1 || x == end - 1) sid[x] = sep;
    else if (x >= end) sid[x] = 0;
    slab[x] = -1;
  }
  __syncthreads();
  if (active) {
    split_lookup(E.S.T, E.S.bytes, E.S.a_off[b], E.S.a_off[b + 1], sid + 1, na, nullptr, E.L);
    split_lookup(E.S.T, E.S.bytes, E.S.b_off[b], E.S.b_off[b + 1], sid + na + 2, nb, nullptr, E.L);
    if (MODE == kPlain && E.G.lab_bytes) {
      // positions count from the sample's [CLS]; one at or past its end would land in the next
      // sample (refused on the host, dropped here)
      const int64_t p0 = E.G.pos_off[b];
      split_lookup(E.S.T, E.G.lab_bytes, E.G.lab_off[b], E.G.lab_off[b + 1], slab,
                   (int32_t)(E.G.pos_off[b + 1] - p0), E.G.pos + p0, end);
    }
  }
  __syncthreads();
  if (!active) return;
  const int64_t o = E.dst[b];
  const int64_t flat = (int64_t)b * E.draw_stride;
  const int64_t seq = E.seq_in_row[b];
  bool carry = false;        // kFusedWw: the state of word_masked, per sample
  int32_t words_before = 0;  // kFusedSpan: that of span_masked, per sample like carry
  uint32_t carry_max = 0;
  // 64-slot windows from the sample's start, the tail predicated: in the two word modes every
  // lane reaches the ballots (and with kFusedSpan the scan) of the word-unit step
  for (int32_t x0 = 0; x0 < fill; x0 += 64) {
    const int32_t x = x0 + lane;
    const bool in = x < fill, real = x < end;
    const bool special = x == 0 || x == na + 1 || x >= end - 1;
    const int32_t id = in ? sid[x] : 0;
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
      if (in && slab[x] >= 0) lab = slab[x];
    }
    if (in) {
      E.input_ids[o + x] = out;
      E.token_type_ids[o + x] = (x >= na + 2 && real) ? 1 : 0;
      E.attention_mask[o + x] = real ? 1 : 0;
      E.position_ids[o + x] = real ? x : 0;
      E.sequence_ids[o + x] = real ? seq : 0;
      if (MODE != kPlain || E.labels) E.labels[o + x] = lab;
      if (MODE == kPlain && E.special_tokens_mask) E.special_tokens_mask[o + x] = special ? 1 : 0;
    }
  }
}

template <int MODE>
int launch(const SeqpackArgs& E, void* stream) {
  return launch_rows(seqpack_kernel<MODE>, E, E.B, 2, E.L, stream);  // ids and labels
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_collate_seqpack(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                    const int64_t* d_a_off, const int64_t* d_b_off,
                                    const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                    const int64_t* d_dst, const int32_t* d_fill,
                                    const int32_t* d_seq_in_row, int32_t max_seq_length,
                                    int64_t* d_input_ids, int64_t* d_token_type_ids,
                                    int64_t* d_attention_mask, int64_t* d_special_tokens_mask,
                                    const uint8_t* d_lab_bytes, const int64_t* d_lab_off,
                                    const uint16_t* d_pos, const int64_t* d_pos_off,
                                    int64_t* d_labels, int64_t ignore_index,
                                    int64_t* d_position_ids, int64_t* d_sequence_ids) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (batch <= 0 || max_seq_length <= 0) return 0;
  if (need_vocab(c, false)) return -1;
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_position_ids ||
      !d_sequence_ids || !d_dst || !d_fill || !d_seq_in_row)
    LDDL_FAIL(-1, "null output");
  const bool is_static = d_lab_bytes != nullptr;
  if (is_static && (!d_lab_off || !d_pos || !d_pos_off || !d_labels || d_special_tokens_mask))
    LDDL_FAIL(-1, "static masking needs its inputs and labels, and no special_tokens_mask");
  if (!is_static && (!d_special_tokens_mask || d_labels))
    LDDL_FAIL(-1, "null output: dynamic masking writes special_tokens_mask, and no labels");
  SeqpackArgs E{{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb}, d_dst, d_fill, d_seq_in_row,
                batch, max_seq_length, d_input_ids, d_token_type_ids, d_attention_mask,
                d_position_ids, d_sequence_ids, d_labels, d_special_tokens_mask,
                {d_lab_bytes, d_lab_off, d_pos, d_pos_off}, ignore_index, 0, {}, {}, {}};
  return launch<kPlain>(E, stream);
}

// lddl_collate_seqpack_masked and, with the span arguments (already validated),
// lddl_collate_seqpack_masked_span
static int seqpack_masked(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                          const int64_t* d_a_off, const int64_t* d_b_off, const int32_t* d_na,
                          const int32_t* d_nb, int32_t batch, const int64_t* d_dst,
                          const int32_t* d_fill, const int32_t* d_seq_in_row,
                          int32_t max_seq_length, int32_t draw_stride, int64_t* d_input_ids,
                          int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
                          int64_t* d_position_ids, int64_t* d_sequence_ids, float mlm_probability,
                          int64_t ignore_index, int64_t vocab_len, uint64_t seed, uint64_t counter,
                          bool whole_word, const SpanDraw* span) {
  if (batch <= 0 || max_seq_length <= 0) return 0;
  if (need_vocab(c, true)) return -1;
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels || !d_position_ids ||
      !d_sequence_ids || !d_dst || !d_fill || !d_seq_in_row)
    LDDL_FAIL(-1, "null output");
  SeqpackArgs E{{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb}, d_dst, d_fill, d_seq_in_row,
                batch, max_seq_length, d_input_ids, d_token_type_ids, d_attention_mask,
                d_position_ids, d_sequence_ids, d_labels, nullptr, {}, ignore_index, draw_stride,
                mask_draw_of(c, mlm_probability, ignore_index, vocab_len, seed, counter),
                cont_bits_of(c), span ? *span : SpanDraw{}};
  switch (fused_mode(whole_word, span)) {
    case kFusedSpan: return launch<kFusedSpan>(E, stream);
    case kFusedWw: return launch<kFusedWw>(E, stream);
    default: return launch<kFused>(E, stream);
  }
}

extern "C" int lddl_collate_seqpack_masked(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                           const int64_t* d_a_off, const int64_t* d_b_off,
                                           const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                           const int64_t* d_dst, const int32_t* d_fill,
                                           const int32_t* d_seq_in_row, int32_t max_seq_length,
                                           int32_t draw_stride, int64_t* d_input_ids,
                                           int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                           int64_t* d_labels, int64_t* d_position_ids,
                                           int64_t* d_sequence_ids, float mlm_probability,
                                           int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                           uint64_t counter, int32_t whole_word) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  return seqpack_masked(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, d_dst, d_fill,
                        d_seq_in_row, max_seq_length, draw_stride, d_input_ids, d_token_type_ids,
                        d_attention_mask, d_labels, d_position_ids, d_sequence_ids, mlm_probability,
                        ignore_index, vocab_len, seed, counter, whole_word != 0, nullptr);
}

extern "C" int lddl_collate_seqpack_masked_span(
    lddl_ctx* c, void* stream, const uint8_t* d_bytes, const int64_t* d_a_off,
    const int64_t* d_b_off, const int32_t* d_na, const int32_t* d_nb, int32_t batch,
    const int64_t* d_dst, const int32_t* d_fill, const int32_t* d_seq_in_row,
    int32_t max_seq_length, int32_t draw_stride, int64_t* d_input_ids, int64_t* d_token_type_ids,
    int64_t* d_attention_mask, int64_t* d_labels, int64_t* d_position_ids,
    int64_t* d_sequence_ids, float mlm_probability, int64_t ignore_index, int64_t vocab_len,
    uint64_t seed, uint64_t counter, const lddl_span_params* params) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  SpanDraw S;
  if (span_draw_of(params, seed, &S)) return -1;
  return seqpack_masked(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, d_dst, d_fill,
                        d_seq_in_row, max_seq_length, draw_stride, d_input_ids, d_token_type_ids,
                        d_attention_mask, d_labels, d_position_ids, d_sequence_ids, mlm_probability,
                        ignore_index, vocab_len, seed, counter, true, &S);
}
