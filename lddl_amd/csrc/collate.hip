// Loader-side collate + dynamic masking (lddl/torch/bert.py:69-196) on the GPU.
//
//   lddl_collate_encode   _to_encoded_inputs (bert.py:69-149): whitespace-split the A / B strings
//                         of a batch, convert_tokens_to_ids (exact vocab lookup, [UNK] if absent),
//                         fill input_ids / token_type_ids / attention_mask and either
//                         special_tokens_mask (dynamic) or labels from masked_lm_positions /
//                         masked_lm_labels (static). One wave per sample.
//   lddl_collate_encode_mp   the same with static masking plus the [B, L] loss mask of
//                         lddl/torch_mp/bert.py:103-105 (1 at masked_lm_positions), written in
//                         the same output loop.
//   lddl_mask_dynamic     _mask_tokens (bert.py:152-196): per slot masked ~ Bernoulli(p) unless
//                         special; of the masked, Bernoulli(0.8) -> [MASK], else Bernoulli(0.5) ->
//                         random id in [0, len(tokenizer)), else unchanged; labels = id where
//                         masked, ignore_index elsewhere. Native mode draws from a counter-based
//                         Philox4x32-10 keyed by (seed, counter, slot); replay mode applies
//                         captured torch masks bit for bit.
//   lddl_collate_encode_masked   _to_encoded_inputs + _mask_tokens in ONE pass (the loader's
//                         dynamic-masking collate, bert.py:348-365): the row is built in LDS and
//                         masked on its way out, so input_ids / token_type_ids / attention_mask /
//                         labels are each written once (36 B per slot incl. the string read)
//                         and no special_tokens_mask is materialised; bit-identical to
//                         lddl_collate_encode followed by lddl_mask_dynamic (same Philox stream).
//   lddl_mask_dynamic_ww / lddl_collate_encode_masked_ww   the same two with whole-word masking
//                         (DESIGN §15): a word = a head plus the continuation ("##x") ids behind
//                         it, and the word's masked / not masked decision is its head's draw. One
//                         wave per row, heads found by ballot; instantiations of their own, the
//                         plain ones are untouched.
//   lddl_mask_dynamic_span / lddl_collate_encode_masked_span   the same two with n-gram (span)
//                         masking: whole words in runs of up to n, the run's reach
//                         carried along the row as a wave prefix maximum (span_dev.h). The
//                         whole-word kernels' other instantiation: one window loop per kernel,
//                         the two modes apart in the one line of the decision.
//
// collate_dev.h holds what this unit shares with the other three collate units (the lookups, the
// masking decision, the string-side arguments StrSample / StrLabels, SlotLayout for mask_special),
// collate_host.h the host side of the entry points (the vocab check, the launch with its LDS
// bound). encode_kernel owns its LDS staging, its two output loops (per token, and one for both
// word modes) and their predicates, written out as in seqpack_kernel: collate_dev.h's comment at
// SlotLayout says why.
#include "collate_host.h"  // need_vocab, mask_draw_of, launch_rows; collate_dev.h
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

struct EncodeArgs {
  static constexpr int kMode = kPlain;
  StrSample S;
  int32_t B, L;
  int64_t* input_ids;
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* special_tokens_mask;  // dynamic masking (nullable)
  StrLabels G;
  int64_t* labels;
  int64_t* loss_mask;  // static masking (nullable): 1 at the sample's masked_lm_positions, else 0
  int64_t ignore_index;
  int32_t fused_mask;  // 1: dynamic masking applied on the way out (labels written from it)
  MaskDraw draw;
};

// One wave per sample; the row is staged in LDS (ids, labels as int32) in two barrier-separated
// phases so that every output element is written exactly once, coalesced.
// The argument struct says the MODE (kMode), the enum of the other three collate kernels.
// EncodeArgs, kPlain, is the kernel as it was, arguments and code: unmasked, static, and the
// per-token fused masking too, which it takes from fused_mask at run time (there is no kFused
// instantiation). EncodeWwArgs, kFusedWw: the fused masking is whole-word and the arguments carry
// the continuation bitmap. EncodeSpanArgs, kFusedSpan: it is the n-gram one and they carry its
// SpanDraw as well. (The kernel is a template over the struct and not over MODE with the struct
// computed from it: a kernel's parameter type is part of its mangled name, and an expression
// over the unnamed enum is spelled differently by the host and the device compilation, so that
// the launch would not find the kernel.)
struct EncodeWwArgs : EncodeArgs {
  static constexpr int kMode = kFusedWw;
  ContBits cont;
};
struct EncodeSpanArgs : EncodeWwArgs {
  static constexpr int kMode = kFusedSpan;
  SpanDraw span;
};
template <typename Args>
__global__ void __launch_bounds__(64 * kEncWaves) encode_kernel(Args E) {
  constexpr int MODE = Args::kMode;
  extern __shared__ __attribute__((aligned(16))) int32_t srow[];
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int b = blockIdx.x * kEncWaves + w;
  const bool active = b < E.B;
  int32_t* sid = srow + (size_t)w * 2 * E.L;
  int32_t* slab = sid + E.L;
  const int32_t na = active ? E.S.na[b] : 0, nb = active ? E.S.nb[b] : 0;
  const int32_t end = na + nb + 3;
  const int32_t cls = E.S.T.special_id[kCls], sep = E.S.T.special_id[kSep];
  if (active) {
    for (int32_t x = lane; x < E.L; x += 64) {
      if (x == 0) sid[x] = cls;
      else if (x == na + 1 || x == end - 1) sid[x] = sep;
      else if (x >= end) sid[x] = 0;
      slab[x] = -1;
    }
  }
  __syncthreads();
  if (active) {
    split_lookup(E.S.T, E.S.bytes, E.S.a_off[b], E.S.a_off[b + 1], sid + 1, na, nullptr, E.L);
    split_lookup(E.S.T, E.S.bytes, E.S.b_off[b], E.S.b_off[b + 1], sid + na + 2, nb, nullptr, E.L);
    if (E.labels && E.G.lab_bytes) {  // labels[b, positions] = ids of masked_lm_labels (bert.py:120-125)
      const int64_t p0 = E.G.pos_off[b];
      const int32_t npos = (int32_t)(E.G.pos_off[b + 1] - p0);
      if (E.loss_mask) {
        // the loss mask follows the positions, not "a label was found": mark them -2 in the
        // labels row (still < 0 = ignore_index if the labels string is short). The label ids
        // land on the same LDS words from other lanes of this wave: marks first.
        for (int32_t k = lane; k < npos; k += 64) {
          const int32_t p = E.G.pos[p0 + k];
          if (p < E.L) slab[p] = -2;
        }
        wave_sync();
      }
      split_lookup(E.S.T, E.G.lab_bytes, E.G.lab_off[b], E.G.lab_off[b + 1], slab, npos,
                   E.G.pos + p0, E.L);
    }
  }
  __syncthreads();
  if (!active) return;
  const int64_t row = (int64_t)b * E.L;
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
      const int32_t id = in ? sid[x] : 0;
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
        E.token_type_ids[row + x] = (x >= na + 2 && x < end) ? 1 : 0;
        E.attention_mask[row + x] = x < end ? 1 : 0;
      }
    }
    return;
  }
  for (int32_t x = lane; x < E.L; x += 64) {
    const bool special = x == 0 || x == na + 1 || x >= end - 1;
    if (E.fused_mask) {
      int64_t lab;
      E.input_ids[row + x] = mask_slot(E.draw, row + x, special, sid[x], &lab);
      E.labels[row + x] = lab;
    } else {
      E.input_ids[row + x] = sid[x];
      if (E.labels) E.labels[row + x] = slab[x] < 0 ? E.ignore_index : (int64_t)slab[x];
      if (E.loss_mask) E.loss_mask[row + x] = slab[x] != -1 ? 1 : 0;
    }
    E.token_type_ids[row + x] = (x >= na + 2 && x < end) ? 1 : 0;
    E.attention_mask[row + x] = x < end ? 1 : 0;
    if (E.special_tokens_mask) E.special_tokens_mask[row + x] = special ? 1 : 0;
  }
}

struct MaskArgs {
  int64_t* ids;        // [B, L] in/out
  int64_t* labels;     // [B, L] out
  const int64_t* special;  // [B, L] special_tokens_mask (nullable -> derived from na/nb, or
                           // without lengths from the ids: get_special_tokens_mask)
  const int32_t* na;
  const int32_t* nb;
  int64_t B, L;
  float p;
  int64_t ignore_index, mask_id, vocab_len;
  int32_t special_ids[kNumSpecial];  // [PAD] [UNK] [CLS] [SEP] [MASK] (-1 if absent)
  uint64_t seed, counter;
  // replay (all or none)
  const uint8_t* r_masked;
  const uint8_t* r_replaced;
  const uint8_t* r_random;
  const int64_t* r_words;
};

// special_tokens_mask of slot i = (b, x): the given tensor, else the layout from the lengths,
// else membership of the id in the special ids
__device__ inline bool mask_special(const MaskArgs& M, int64_t i, int64_t b, int64_t x, int64_t id) {
  if (M.special) return M.special[i] != 0;
  if (M.na) {
    const int32_t na = M.na[b], end = na + M.nb[b] + 3;
    return SlotLayout{na, end}.special(x);
  }
  bool sp = false;  // tokenizer.get_special_tokens_mask(ids, already_has_special_tokens=True)
  for (int k = 0; k < kNumSpecial; ++k) sp |= M.special_ids[k] >= 0 && id == M.special_ids[k];
  return sp;
}

__global__ void __launch_bounds__(256) mask_kernel(MaskArgs M) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M.B * M.L) return;
  const int64_t b = i / M.L, x = i - b * M.L;
  const int64_t id = M.ids[i];
  const bool special = mask_special(M, i, b, x, id);
  if (!M.r_masked) {  // native: the shared Philox decision (also used by the fused collate)
    int64_t lab;
    const int64_t out = mask_slot(MaskDraw{M.p, M.ignore_index, M.mask_id, M.vocab_len, M.seed,
                                           M.counter}, i, special, id, &lab);
    M.labels[i] = lab;
    if (out != id) M.ids[i] = out;
    return;
  }
  // replay of captured torch draws: masked_indices already excludes special slots
  const bool masked = M.r_masked[i], replaced = M.r_replaced[i], rnd = M.r_random[i];
  M.labels[i] = masked ? id : M.ignore_index;
  if (replaced) M.ids[i] = M.mask_id;
  else if (rnd) M.ids[i] = M.r_words[i];
}

constexpr int kWwWaves = 4;

// Whole-word (mask_words_kernel<kFusedWw>) and n-gram (<kFusedSpan, SpanDraw>) lddl_mask_dynamic:
// one wave per row (a word never leaves its row), 64-slot windows. The special flag of slot x - 1
// comes from the lane below, across windows from lane 63. Span is the n-gram kernel's third
// argument, SpanDraw; the whole-word kernel has two, as it had. (A pack, not one body under two
// __global__ functions: that form comes out with other code)
template <int MODE, typename... Span>
__global__ void __launch_bounds__(64 * kWwWaves) mask_words_kernel(MaskArgs M, ContBits C,
                                                                   Span... S) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kWwWaves + wave_id();
  if (b >= M.B) return;  // the whole wave
  const MaskDraw D{M.p, M.ignore_index, M.mask_id, M.vocab_len, M.seed, M.counter};
  bool carry = false;        // kFusedWw: the state of word_masked between the row's windows
  int32_t words_before = 0;  // kFusedSpan: that of span_masked
  uint32_t carry_max = 0;
  int last_special = 1;  // slot 0 has no slot before it: never a continuation
  for (int64_t x0 = 0; x0 < M.L; x0 += 64) {
    const int64_t x = x0 + lane, i = b * M.L + x;
    const bool in = x < M.L;
    const int64_t id = in ? M.ids[i] : 0;
    const bool special = !in || mask_special(M, i, b, x, id);
    const int up = __shfl_up((int)special, 1, 64);
    const bool prev_special = lane == 0 ? last_special != 0 : up != 0;
    last_special = __shfl((int)special, 63, 64);
    const bool cont = !special && !prev_special && cont_id(C, id);
    const uint4 r = mask_draw(D, i);
    bool m;  // the one line in which the two word modes differ
    if constexpr (MODE == kFusedSpan)
      m = span_masked(S..., D.counter, !special && !cont, r, i, words_before, carry_max);
    else
      m = word_masked(!cont, u01(r.x) < D.p, lane, carry);
    if (in) {
      int64_t lab;
      const int64_t out = mask_apply(D, r, !special && m, id, &lab);
      M.labels[i] = lab;
      if (out != id) M.ids[i] = out;
    }
  }
}

}  // namespace
}  // namespace lddl

using namespace lddl;

// lddl_collate_encode (d_loss_mask == nullptr) and lddl_collate_encode_mp
static int collate_encode(lddl_ctx* c, void* stream, const uint8_t* d_bytes, const int64_t* d_a_off,
                          const int64_t* d_b_off, const int32_t* d_na, const int32_t* d_nb,
                          int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                          int64_t* d_token_type_ids, int64_t* d_attention_mask,
                          int64_t* d_special_tokens_mask, const uint8_t* d_lab_bytes,
                          const int64_t* d_lab_off, const uint16_t* d_pos, const int64_t* d_pos_off,
                          int64_t* d_labels, int64_t* d_loss_mask, int64_t ignore_index) {
  if (batch <= 0 || seq_len <= 0) return 0;
  if (need_vocab(c, false)) return -1;
  EncodeArgs E{{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb}, batch, seq_len, d_input_ids,
               d_token_type_ids, d_attention_mask, d_special_tokens_mask,
               {d_lab_bytes, d_lab_off, d_pos, d_pos_off}, d_labels, d_loss_mask, ignore_index, 0,
               {}};
  return launch_rows(encode_kernel<EncodeArgs>, E, batch, 2, seq_len, stream);  // ids and labels
}

// lddl_collate_encode_masked, lddl_collate_encode_masked_ww and (span given)
// lddl_collate_encode_masked_span
static int collate_encode_masked(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                 const int64_t* d_a_off, const int64_t* d_b_off,
                                 const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                 int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids,
                                 int64_t* d_attention_mask, int64_t* d_labels,
                                 float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                                 uint64_t seed, uint64_t counter, bool whole_word,
                                 const SpanDraw* span = nullptr) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (batch <= 0 || seq_len <= 0) return 0;
  if (need_vocab(c, true)) return -1;
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels)
    LDDL_FAIL(-1, "null output");
  const EncodeSpanArgs E{{{{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb}, batch, seq_len,
                           d_input_ids, d_token_type_ids, d_attention_mask, nullptr, {}, d_labels,
                           nullptr, ignore_index, 1,
                           mask_draw_of(c, mlm_probability, ignore_index, vocab_len, seed,
                                        counter)},
                          cont_bits_of(c)},
                         span ? *span : SpanDraw{}};
  const EncodeWwArgs& W = E;  // each kernel takes the part of E it was written for
  const EncodeArgs& P = E;
  switch (fused_mode(whole_word, span)) {
    case kFusedSpan:
      return launch_rows(encode_kernel<EncodeSpanArgs>, E, batch, 2, seq_len, stream);
    case kFusedWw: return launch_rows(encode_kernel<EncodeWwArgs>, W, batch, 2, seq_len, stream);
    default: return launch_rows(encode_kernel<EncodeArgs>, P, batch, 2, seq_len, stream);  // kFused
  }
}

extern "C" int lddl_collate_encode(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                   const int64_t* d_a_off, const int64_t* d_b_off,
                                   const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                   int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids,
                                   int64_t* d_attention_mask, int64_t* d_special_tokens_mask,
                                   const uint8_t* d_lab_bytes, const int64_t* d_lab_off,
                                   const uint16_t* d_pos, const int64_t* d_pos_off,
                                   int64_t* d_labels, int64_t ignore_index) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  return collate_encode(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len,
                        d_input_ids, d_token_type_ids, d_attention_mask, d_special_tokens_mask,
                        d_lab_bytes, d_lab_off, d_pos, d_pos_off, d_labels, nullptr, ignore_index);
}

extern "C" int lddl_collate_encode_mp(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                      const int64_t* d_a_off, const int64_t* d_b_off,
                                      const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                      int32_t seq_len, int64_t* d_input_ids,
                                      int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                      int64_t* d_special_tokens_mask, const uint8_t* d_lab_bytes,
                                      const int64_t* d_lab_off, const uint16_t* d_pos,
                                      const int64_t* d_pos_off, int64_t* d_labels,
                                      int64_t ignore_index, int64_t* d_loss_mask) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (!d_loss_mask) LDDL_FAIL(-1, "null loss mask");
  if (!d_lab_bytes || !d_lab_off || !d_pos || !d_pos_off || !d_labels)
    LDDL_FAIL(-1, "the loss mask needs the static-masking inputs and labels");
  return collate_encode(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len,
                        d_input_ids, d_token_type_ids, d_attention_mask, d_special_tokens_mask,
                        d_lab_bytes, d_lab_off, d_pos, d_pos_off, d_labels, d_loss_mask,
                        ignore_index);
}

// What the three lddl_mask_dynamic* entry points refuse, in their order, and the arguments of
// their kernels (native mode: lddl_mask_dynamic adds its replay pointers). An empty batch is
// refused like a full one; each entry point returns 0 for it afterwards, by its own rule.
static int mask_args_of(lddl_ctx* c, int64_t* d_input_ids, int64_t* d_labels,
                        const int64_t* d_special_tokens_mask, const int32_t* d_na,
                        const int32_t* d_nb, int64_t batch, int64_t seq_len, float mlm_probability,
                        int64_t ignore_index, int64_t vocab_len, uint64_t seed, uint64_t counter,
                        MaskArgs* M) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (!d_special_tokens_mask && (!d_na != !d_nb)) LDDL_FAIL(-1, "need both lengths or neither");
  if (c->tab.special_id[kMask] < 0) LDDL_FAIL(-1, "vocab has no [MASK]");
  *M = MaskArgs{d_input_ids, d_labels, d_special_tokens_mask, d_na, d_nb, batch, seq_len,
                mlm_probability, ignore_index, c->tab.special_id[kMask], vocab_len, {}, seed,
                counter, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < kNumSpecial; ++k) M->special_ids[k] = c->tab.special_id[k];
  return 0;
}

// mask_words_kernel over M's rows, kWwWaves of them per block; S: the span arguments, or nothing
template <int MODE, typename... Span>
static int launch_mask_words(lddl_ctx* c, void* stream, const MaskArgs& M, const Span&... S) {
  hipLaunchKernelGGL((mask_words_kernel<MODE, Span...>),
                     dim3((unsigned)((M.B + kWwWaves - 1) / kWwWaves)), dim3(64 * kWwWaves), 0,
                     as_stream(stream), M, cont_bits_of(c), S...);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_mask_dynamic(lddl_ctx* c, void* stream, int64_t* d_input_ids, int64_t* d_labels,
                                 const int64_t* d_special_tokens_mask, const int32_t* d_na,
                                 const int32_t* d_nb, int64_t batch, int64_t seq_len,
                                 float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                                 uint64_t seed, uint64_t counter, const uint8_t* d_r_masked,
                                 const uint8_t* d_r_replaced, const uint8_t* d_r_random,
                                 const int64_t* d_r_words) {
  MaskArgs M;
  if (mask_args_of(c, d_input_ids, d_labels, d_special_tokens_mask, d_na, d_nb, batch, seq_len,
                   mlm_probability, ignore_index, vocab_len, seed, counter, &M))
    return -1;
  const int64_t n = batch * seq_len;
  if (n <= 0) return 0;
  M.r_masked = d_r_masked, M.r_replaced = d_r_replaced, M.r_random = d_r_random;
  M.r_words = d_r_words;
  hipLaunchKernelGGL(mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), M);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_collate_encode_masked(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                          const int64_t* d_a_off, const int64_t* d_b_off,
                                          const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                          int32_t seq_len, int64_t* d_input_ids,
                                          int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                          int64_t* d_labels, float mlm_probability,
                                          int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                          uint64_t counter) {
  return collate_encode_masked(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len,
                               d_input_ids, d_token_type_ids, d_attention_mask, d_labels,
                               mlm_probability, ignore_index, vocab_len, seed, counter, false);
}

extern "C" int lddl_mask_dynamic_ww(lddl_ctx* c, void* stream, int64_t* d_input_ids,
                                    int64_t* d_labels, const int64_t* d_special_tokens_mask,
                                    const int32_t* d_na, const int32_t* d_nb, int64_t batch,
                                    int64_t seq_len, float mlm_probability, int64_t ignore_index,
                                    int64_t vocab_len, uint64_t seed, uint64_t counter) {
  MaskArgs M;
  if (mask_args_of(c, d_input_ids, d_labels, d_special_tokens_mask, d_na, d_nb, batch, seq_len,
                   mlm_probability, ignore_index, vocab_len, seed, counter, &M))
    return -1;
  if (batch <= 0 || seq_len <= 0) return 0;
  return launch_mask_words<kFusedWw>(c, stream, M);
}

extern "C" int lddl_collate_encode_masked_ww(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                             const int64_t* d_a_off, const int64_t* d_b_off,
                                             const int32_t* d_na, const int32_t* d_nb,
                                             int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                                             int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                             int64_t* d_labels, float mlm_probability,
                                             int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                             uint64_t counter) {
  return collate_encode_masked(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len,
                               d_input_ids, d_token_type_ids, d_attention_mask, d_labels,
                               mlm_probability, ignore_index, vocab_len, seed, counter, true);
}

extern "C" int lddl_mask_dynamic_span(lddl_ctx* c, void* stream, int64_t* d_input_ids,
                                      int64_t* d_labels, const int64_t* d_special_tokens_mask,
                                      const int32_t* d_na, const int32_t* d_nb, int64_t batch,
                                      int64_t seq_len, float mlm_probability, int64_t ignore_index,
                                      int64_t vocab_len, uint64_t seed, uint64_t counter,
                                      const lddl_span_params* params) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  SpanDraw S;
  if (span_draw_of(params, seed, &S)) return -1;
  MaskArgs M;
  if (mask_args_of(c, d_input_ids, d_labels, d_special_tokens_mask, d_na, d_nb, batch, seq_len,
                   mlm_probability, ignore_index, vocab_len, seed, counter, &M))
    return -1;
  if (batch <= 0 || seq_len <= 0) return 0;
  return launch_mask_words<kFusedSpan>(c, stream, M, S);
}

extern "C" int lddl_collate_encode_masked_span(
    lddl_ctx* c, void* stream, const uint8_t* d_bytes, const int64_t* d_a_off,
    const int64_t* d_b_off, const int32_t* d_na, const int32_t* d_nb, int32_t batch,
    int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids, int64_t* d_attention_mask,
    int64_t* d_labels, float mlm_probability, int64_t ignore_index, int64_t vocab_len,
    uint64_t seed, uint64_t counter, const lddl_span_params* params) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  SpanDraw S;
  if (span_draw_of(params, seed, &S)) return -1;
  return collate_encode_masked(c, stream, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len,
                               d_input_ids, d_token_type_ids, d_attention_mask, d_labels,
                               mlm_probability, ignore_index, vocab_len, seed, counter, true, &S);
}
