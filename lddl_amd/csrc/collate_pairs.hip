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
// and the masking decision of a slot is collate_dev.h's (MaskDraw, mask_draw, mask_apply,
// word_masked, ContBits), with the same Philox index i * seq_len + x: the mask stream is the
// string kernels' by construction.
//
//   lddl_collate_pairs          lddl_collate_encode: unmasked (special_tokens_mask) or static
//                               (labels scattered from pos / labels through one LDS row per wave,
//                               so that labels too are written once, coalesced)
//   lddl_collate_pairs_masked   lddl_collate_encode_masked / _masked_ww (no LDS at all)
//
// One wave per output row, kEncWaves rows per block; all offsets 64-bit (a table holds more than
// 2^31 tokens); both id widths of lddl_ctx_id_bytes().
#include "collate_dev.h"  // MaskDraw ..., ContBits, word_masked, kEncWaves
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

enum { kPlain = 0, kFused = 1, kFusedWw = 2 };

struct PairsArgs {
  const void* tokens;      // uint16 or int32 ids
  const int64_t* tok_off;  // [n_pairs + 1]
  const int32_t* len_a;
  const uint8_t* is_rn;
  // static masking (all or none)
  const uint16_t* pos;
  const void* lab;
  const int64_t* pos_off;
  const int64_t* rows;  // nullable: identity
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
};

template <typename ID>
__device__ inline int32_t load_id(const void* p, int64_t i) {
  return (int32_t) reinterpret_cast<const ID*>(p)[i];
}

template <typename ID, int MODE>
__global__ void __launch_bounds__(64 * kEncWaves) pairs_kernel(PairsArgs E) {
  extern __shared__ __attribute__((aligned(16))) int32_t srow[];  // static masking: [waves][L]
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int32_t b = blockIdx.x * kEncWaves + w;
  if (b >= E.B) return;  // the whole wave; no block-wide barrier below
  const int64_t q = E.rows ? E.rows[b] : (int64_t)b;
  const int64_t t0 = E.tok_off[q];
  const int32_t na = E.len_a[q];
  const int32_t nb = (int32_t)(E.tok_off[q + 1] - t0) - na;
  const int32_t end = na + nb + 3;
  const int64_t row = (int64_t)b * E.L;
  if (lane == 0) E.nsl[b] = E.is_rn[q] ? 1 : 0;

  // the slot's id before masking (x < L)
  auto slot_id = [&](int32_t x) -> int32_t {
    if (x == 0) return E.cls;
    if (x == na + 1 || x == end - 1) return E.sep;
    if (x >= end) return 0;
    return load_id<ID>(E.tokens, t0 + x - (x <= na ? 1 : 2));
  };

  if constexpr (MODE == kFusedWw) {
    // windows of 64 slots up to a multiple of 64, the tail predicated: every lane reaches the
    // ballots of word_masked
    bool carry = false;
    for (int32_t x0 = 0; x0 < E.L; x0 += 64) {
      const int32_t x = x0 + lane;
      const bool in = x < E.L;
      const bool special = x == 0 || x == na + 1 || x >= end - 1;
      const bool prev_special = x <= 1 || x - 1 == na + 1 || x - 1 >= end - 1;  // of slot x - 1
      const int32_t id = in ? slot_id(x) : 0;
      const bool cont = in && !special && !prev_special && cont_id(E.cont, id);
      const uint4 r = mask_draw(E.draw, row + x);
      const bool m = word_masked(!cont, u01(r.x) < E.draw.p, lane, carry);
      if (in) {
        int64_t lab;
        E.input_ids[row + x] = mask_apply(E.draw, r, !special && m, id, &lab);
        E.labels[row + x] = lab;
        E.token_type_ids[row + x] = (x >= na + 2 && x < end) ? 1 : 0;
        E.attention_mask[row + x] = x < end ? 1 : 0;
      }
    }
    return;
  } else if constexpr (MODE == kFused) {
    for (int32_t x = lane; x < E.L; x += 64) {
      const bool special = x == 0 || x == na + 1 || x >= end - 1;
      const uint4 r = mask_draw(E.draw, row + x);
      int64_t lab;
      E.input_ids[row + x] =
          mask_apply(E.draw, r, !special && u01(r.x) < E.draw.p, slot_id(x), &lab);
      E.labels[row + x] = lab;
      E.token_type_ids[row + x] = (x >= na + 2 && x < end) ? 1 : 0;
      E.attention_mask[row + x] = x < end ? 1 : 0;
    }
    return;
  } else {
    int32_t* slab = srow + (size_t)w * E.L;
    if (E.pos) {  // labels[b, positions] = the pair's label ids; a position >= L is dropped
      for (int32_t x = lane; x < E.L; x += 64) slab[x] = -1;
      wave_sync();
      const int64_t p0 = E.pos_off[q];
      const int32_t npos = (int32_t)(E.pos_off[q + 1] - p0);
      for (int32_t k = lane; k < npos; k += 64) {
        const int32_t p = E.pos[p0 + k];
        if (p < E.L) slab[p] = load_id<ID>(E.lab, p0 + k);
      }
      wave_sync();
    }
    for (int32_t x = lane; x < E.L; x += 64) {
      E.input_ids[row + x] = slot_id(x);
      E.token_type_ids[row + x] = (x >= na + 2 && x < end) ? 1 : 0;
      E.attention_mask[row + x] = x < end ? 1 : 0;
      if (E.pos) E.labels[row + x] = slab[x] < 0 ? E.ignore_index : (int64_t)slab[x];
      else E.special_tokens_mask[row + x] = (x == 0 || x == na + 1 || x >= end - 1) ? 1 : 0;
    }
  }
}

template <int MODE>
int launch(lddl_ctx* c, const PairsArgs& E, void* stream) {
  const size_t lds = (MODE == kPlain && E.pos) ? sizeof(int32_t) * (size_t)E.L * kEncWaves : 0;
  if (lds > 160 * 1024) LDDL_FAIL(-1, "sequence length %d too long for the collate kernel", E.L);
  const dim3 grid((unsigned)((E.B + kEncWaves - 1) / kEncWaves)), block(64 * kEncWaves);
  if (c->id_bytes() == 2)
    hipLaunchKernelGGL((pairs_kernel<uint16_t, MODE>), grid, block, lds, as_stream(stream), E);
  else
    hipLaunchKernelGGL((pairs_kernel<int32_t, MODE>), grid, block, lds, as_stream(stream), E);
  LDDL_HIP(hipGetLastError());
  return 0;
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
  if (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0)
    LDDL_FAIL(-1, "vocab needs [CLS] and [SEP]");
  if (!d_tokens || !d_tok_off || !d_len_a || !d_is_rn) LDDL_FAIL(-1, "null pair table");
  const bool is_static = d_pos != nullptr;
  if ((d_lab != nullptr) != is_static || (d_pos_off != nullptr) != is_static)
    LDDL_FAIL(-1, "static masking needs pos, labels and pos_off, all three or none");
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_next_sentence_labels ||
      (is_static ? !d_labels : !d_special_tokens_mask))
    LDDL_FAIL(-1, "null output");
  PairsArgs E{d_tokens, d_tok_off, d_len_a, d_is_rn, d_pos, d_lab, d_pos_off, d_rows, batch,
              seq_len, c->tab.special_id[kCls], c->tab.special_id[kSep], d_input_ids,
              d_token_type_ids, d_attention_mask, d_special_tokens_mask, d_labels,
              d_next_sentence_labels, ignore_index, {}, {}};
  return launch<kPlain>(c, E, stream);
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
  if (batch <= 0 || seq_len <= 0) return 0;
  if (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0 || c->tab.special_id[kMask] < 0)
    LDDL_FAIL(-1, "vocab needs [CLS], [SEP] and [MASK]");
  if (!d_tokens || !d_tok_off || !d_len_a || !d_is_rn) LDDL_FAIL(-1, "null pair table");
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels ||
      !d_next_sentence_labels)
    LDDL_FAIL(-1, "null output");
  PairsArgs E{d_tokens, d_tok_off, d_len_a, d_is_rn, nullptr, nullptr, nullptr, d_rows, batch,
              seq_len, c->tab.special_id[kCls], c->tab.special_id[kSep], d_input_ids,
              d_token_type_ids, d_attention_mask, nullptr, d_labels, d_next_sentence_labels,
              ignore_index,
              MaskDraw{mlm_probability, ignore_index, c->tab.special_id[kMask], vocab_len, seed,
                       counter},
              ContBits{c->d_cont_bits, c->vocab_size}};
  return whole_word ? launch<kFusedWw>(c, E, stream) : launch<kFused>(c, E, stream);
}
