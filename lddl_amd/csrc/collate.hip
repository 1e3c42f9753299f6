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
//                         wave per row, heads found by ballot; kernels of their own, the plain
//                         ones are untouched.
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

#include <type_traits>

namespace lddl {
namespace {

__device__ inline float u01(uint32_t x) { return (x >> 8) * (1.0f / 16777216.0f); }

// exact token string -> id (convert_tokens_to_ids); "##x" is the continuation entry of "x"
__device__ int32_t token_lookup(const Tables& T, const uint8_t* s, int len) {
  uint32_t cont = 0;
  if (len > 2 && s[0] == '#' && s[1] == '#') { cont = 1; s += 2; len -= 2; }
  if (len > 255) return -1;
  uint64_t k0 = 0;
  uint32_t k1 = 0;
  for (int i = 0; i < len && i < 8; ++i) k0 |= (uint64_t)s[i] << (8 * i);
  for (int i = 8; i < len && i < 12; ++i) k1 |= (uint32_t)s[i] << (8 * (i - 8));
  const uint32_t want = kMetaValid | (cont ? kMetaCont : 0u) | (len > 12 ? kMetaLong : 0u) |
                        ((uint32_t)len << 21);
  for (uint32_t slot = (uint32_t)vhash(k0, k1, len, cont) & T.vmask;; slot = (slot + 1) & T.vmask) {
    const VEnt e = T.vhash[slot];
    if (!(e.meta & kMetaValid)) return -1;
    if (e.k0 == k0 && e.k1 == k1 && (e.meta & ~0x1FFFFFu) == want) {
      const int32_t id = meta_id(e.meta);
      if (len <= 12) return id;
      const uint8_t* p = T.vbytes + T.voff[id];
      bool ok = true;
      for (int i = 12; i < len; ++i) ok &= p[i] == s[i];
      if (ok) return id;
    }
  }
}

__device__ inline bool is_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

// Split bytes[b0,b1) on whitespace and look every token up; token t -> out[t] (t < max_tok).
// Whole wave cooperates: 64-byte windows, word starts found by ballot. Returns #tokens.
__device__ int32_t split_lookup(const Tables& T, const uint8_t* bytes, int64_t b0, int64_t b1,
                                int32_t* out, int32_t max_tok, const uint16_t* scatter,
                                int32_t limit) {
  const int lane = lane_id();
  int32_t ntok = 0;
  uint8_t prev = ' ';
  for (int64_t base = b0; base < b1; base += 64) {
    const int64_t i = base + lane;
    const uint8_t c = i < b1 ? bytes[i] : ' ';
    const int up = __shfl_up((int)c, 1, 64);  // every lane must take part in the shuffle
    const uint8_t pc = lane == 0 ? prev : (uint8_t)up;
    const bool start = !is_ws(c) && is_ws(pc);
    const uint64_t m = __ballot(start);
    if (start) {
      const int32_t t = ntok + __popcll(m & ((1ull << lane) - 1));
      int64_t e = i;
      while (e < b1 && !is_ws(bytes[e])) ++e;
      int32_t id = token_lookup(T, bytes + i, (int)(e - i));
      if (id < 0) id = T.special_id[kUnk];
      if (t < max_tok) {
        const int32_t dst = scatter ? (int32_t)scatter[t] : t;
        if (dst < limit) out[dst] = id;  // a masked position >= L is refused on the host
      }
    }
    ntok += __popcll(m);
    prev = (uint8_t)__shfl((int)c, 63, 64);
  }
  return ntok;
}

// One slot's native-RNG masking decision (bert.py:176-192): Philox4x32-10 keyed by seed, counter
// (batch) and the flat slot index. Returns the output id; *label = id if masked else ignore.
struct MaskDraw {
  float p;
  int64_t ignore_index, mask_id, vocab_len;
  uint64_t seed, counter;
};
__device__ inline uint4 mask_draw(const MaskDraw& D, int64_t flat) {
  return Philox::gen(make_uint4((uint32_t)flat, (uint32_t)(flat >> 32), (uint32_t)D.counter,
                                (uint32_t)(D.counter >> 32)),
                     make_uint2((uint32_t)D.seed, (uint32_t)(D.seed >> 32)));
}
// the slot's outcome once `masked` is decided: 80 / 10 / 10 and the random id from its own draw
__device__ inline int64_t mask_apply(const MaskDraw& D, const uint4 r, bool masked, int64_t id,
                                     int64_t* label) {
  const bool replaced = masked && u01(r.y) < 0.8f;
  const bool rnd = masked && !replaced && u01(r.z) < 0.5f;
  *label = masked ? id : D.ignore_index;
  if (replaced) return D.mask_id;
  if (rnd) return (int64_t)(((uint64_t)r.w * (uint64_t)D.vocab_len) >> 32);
  return id;
}
__device__ inline int64_t mask_slot(const MaskDraw& D, int64_t flat, bool special, int64_t id,
                                    int64_t* label) {
  const uint4 r = mask_draw(D, flat);
  return mask_apply(D, r, !special && u01(r.x) < D.p, id, label);
}

// Whole-word masking. A slot is a continuation iff it and the slot before it are
// not special and its id is a "##x" vocab entry (the context's per-id bitmap: ids, not strings,
// so an unknown "##zzz" that became [UNK] is a head). A word's decision is its head's draw.
struct ContBits {
  const uint32_t* bits;  // bit id of word id >> 5
  int32_t vocab_size;
};
__device__ inline bool cont_id(const ContBits& C, int64_t id) {
  return id >= 0 && id < C.vocab_size && ((C.bits[id >> 5] >> (id & 31)) & 1u);
}
// One 64-slot window of a row, lane = slot, EVERY lane of the wave calls it (two ballots; lanes
// past the row pass head = true, own = false). `own` is the lane's own u01(r.x) < p. Returns the
// decision of the lane's head: the highest head at or below it, or, if the window has none
// there, the last head of the windows before (`carry`, which this call updates).
__device__ inline bool word_masked(bool head, bool own, int lane, bool& carry) {
  const uint64_t heads = __ballot(head);
  const uint64_t dec = __ballot(own);
  const uint64_t below = heads & (~0ull >> (63 - lane));
  bool m = carry;
  if (below) m = (dec >> (63 - __clzll((long long)below))) & 1;
  if (heads) carry = (dec >> (63 - __clzll((long long)heads))) & 1;
  return m;
}

struct EncodeArgs {
  Tables T;
  const uint8_t* bytes;
  const int64_t* a_off;  // [B+1] A string of sample b = bytes[a_off[b], a_off[b+1])
  const int64_t* b_off;  // [B+1]
  const int32_t* na;     // [B] token counts of A / B (host-computed, they size the batch)
  const int32_t* nb;
  int32_t B, L;
  int64_t* input_ids;
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* special_tokens_mask;  // dynamic masking (nullable)
  // static masking (all nullable)
  const uint8_t* lab_bytes;
  const int64_t* lab_off;
  const uint16_t* pos;
  const int64_t* pos_off;
  int64_t* labels;
  int64_t* loss_mask;  // static masking (nullable): 1 at the sample's masked_lm_positions, else 0
  int64_t ignore_index;
  int32_t fused_mask;  // 1: dynamic masking applied on the way out (labels written from it)
  MaskDraw draw;
};

constexpr int kEncWaves = 4;

// One wave per sample; the row is staged in LDS (ids, labels as int32) in two barrier-separated
// phases so that every output element is written exactly once, coalesced.
// WW: the fused masking is whole-word and the arguments carry the continuation bitmap; the
// plain instantiation is the kernel as it was, arguments and code.
struct EncodeWwArgs : EncodeArgs {
  ContBits cont;
};
template <bool WW>
__global__ void __launch_bounds__(64 * kEncWaves)
encode_kernel(std::conditional_t<WW, EncodeWwArgs, EncodeArgs> E) {
  extern __shared__ __attribute__((aligned(16))) int32_t srow[];
  const int w = wave_id(), lane = threadIdx.x & 63;
  const int b = blockIdx.x * kEncWaves + w;
  const bool active = b < E.B;
  int32_t* sid = srow + (size_t)w * 2 * E.L;
  int32_t* slab = sid + E.L;
  const int32_t na = active ? E.na[b] : 0, nb = active ? E.nb[b] : 0;
  const int32_t end = na + nb + 3;
  const int32_t cls = E.T.special_id[kCls], sep = E.T.special_id[kSep];
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
    split_lookup(E.T, E.bytes, E.a_off[b], E.a_off[b + 1], sid + 1, na, nullptr, E.L);
    split_lookup(E.T, E.bytes, E.b_off[b], E.b_off[b + 1], sid + na + 2, nb, nullptr, E.L);
    if (E.labels && E.lab_bytes) {  // labels[b, positions] = ids of masked_lm_labels (bert.py:120-125)
      const int64_t p0 = E.pos_off[b];
      const int32_t npos = (int32_t)(E.pos_off[b + 1] - p0);
      if (E.loss_mask) {
        // the loss mask follows the positions, not "a label was found": mark them -2 in the
        // labels row (still < 0 = ignore_index if the labels string is short). The label ids
        // land on the same LDS words from other lanes of this wave: marks first.
        for (int32_t k = lane; k < npos; k += 64) {
          const int32_t p = E.pos[p0 + k];
          if (p < E.L) slab[p] = -2;
        }
        wave_sync();
      }
      split_lookup(E.T, E.lab_bytes, E.lab_off[b], E.lab_off[b + 1], slab, npos, E.pos + p0, E.L);
    }
  }
  __syncthreads();
  if (!active) return;
  const int64_t row = (int64_t)b * E.L;
  if constexpr (WW) {
    // windows of 64 slots up to a multiple of 64, the tail predicated: every lane reaches the
    // ballots of word_masked
    bool carry = false;
    for (int32_t x0 = 0; x0 < E.L; x0 += 64) {
      const int32_t x = x0 + lane;
      const bool in = x < E.L;
      const bool special = x == 0 || x == na + 1 || x >= end - 1;
      const bool prev_special = x <= 1 || x - 1 == na + 1 || x - 1 >= end - 1;  // of slot x - 1
      const int32_t id = in ? sid[x] : 0;
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
    return x == 0 || x == na + 1 || x >= end - 1;
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

// Whole-word lddl_mask_dynamic: one wave per row (a word never leaves its row), 64-slot windows.
// The special flag of slot x - 1 comes from the lane below, across windows from lane 63.
__global__ void __launch_bounds__(64 * kWwWaves) mask_ww_kernel(MaskArgs M, ContBits C) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kWwWaves + wave_id();
  if (b >= M.B) return;  // the whole wave
  const MaskDraw D{M.p, M.ignore_index, M.mask_id, M.vocab_len, M.seed, M.counter};
  bool carry = false;
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
    const bool m = word_masked(!cont, u01(r.x) < D.p, lane, carry);
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
  if (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0)
    LDDL_FAIL(-1, "vocab needs [CLS] and [SEP]");
  EncodeArgs E{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len, d_input_ids,
               d_token_type_ids, d_attention_mask, d_special_tokens_mask, d_lab_bytes, d_lab_off,
               d_pos, d_pos_off, d_labels, d_loss_mask, ignore_index, 0, {}};
  const size_t lds = sizeof(int32_t) * 2 * (size_t)seq_len * kEncWaves;
  if (lds > 160 * 1024) LDDL_FAIL(-1, "sequence length %d too long for the collate kernel", seq_len);
  hipLaunchKernelGGL(encode_kernel<false>, dim3((unsigned)((batch + kEncWaves - 1) / kEncWaves)),
                     dim3(64 * kEncWaves), lds, as_stream(stream), E);
  LDDL_HIP(hipGetLastError());
  return 0;
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

extern "C" int lddl_mask_dynamic(lddl_ctx* c, void* stream, int64_t* d_input_ids, int64_t* d_labels,
                                 const int64_t* d_special_tokens_mask, const int32_t* d_na,
                                 const int32_t* d_nb, int64_t batch, int64_t seq_len,
                                 float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                                 uint64_t seed, uint64_t counter, const uint8_t* d_r_masked,
                                 const uint8_t* d_r_replaced, const uint8_t* d_r_random,
                                 const int64_t* d_r_words) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (!d_special_tokens_mask && (!d_na != !d_nb)) LDDL_FAIL(-1, "need both lengths or neither");
  if (c->tab.special_id[kMask] < 0) LDDL_FAIL(-1, "vocab has no [MASK]");
  const int64_t n = batch * seq_len;
  if (n <= 0) return 0;
  MaskArgs M{d_input_ids, d_labels, d_special_tokens_mask, d_na, d_nb, batch, seq_len,
             mlm_probability, ignore_index, c->tab.special_id[kMask], vocab_len, {}, seed, counter,
             d_r_masked, d_r_replaced, d_r_random, d_r_words};
  for (int k = 0; k < kNumSpecial; ++k) M.special_ids[k] = c->tab.special_id[k];
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
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (batch <= 0 || seq_len <= 0) return 0;
  if (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0 || c->tab.special_id[kMask] < 0)
    LDDL_FAIL(-1, "vocab needs [CLS], [SEP] and [MASK]");
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels)
    LDDL_FAIL(-1, "null output");
  EncodeArgs E{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len, d_input_ids,
               d_token_type_ids, d_attention_mask, nullptr, nullptr, nullptr, nullptr, nullptr,
               d_labels, nullptr, ignore_index, 1,
               MaskDraw{mlm_probability, ignore_index, c->tab.special_id[kMask], vocab_len, seed,
                        counter}};
  const size_t lds = sizeof(int32_t) * 2 * (size_t)seq_len * kEncWaves;
  if (lds > 160 * 1024) LDDL_FAIL(-1, "sequence length %d too long for the collate kernel", seq_len);
  hipLaunchKernelGGL(encode_kernel<false>, dim3((unsigned)((batch + kEncWaves - 1) / kEncWaves)),
                     dim3(64 * kEncWaves), lds, as_stream(stream), E);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_mask_dynamic_ww(lddl_ctx* c, void* stream, int64_t* d_input_ids,
                                    int64_t* d_labels, const int64_t* d_special_tokens_mask,
                                    const int32_t* d_na, const int32_t* d_nb, int64_t batch,
                                    int64_t seq_len, float mlm_probability, int64_t ignore_index,
                                    int64_t vocab_len, uint64_t seed, uint64_t counter) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (!d_special_tokens_mask && (!d_na != !d_nb)) LDDL_FAIL(-1, "need both lengths or neither");
  if (c->tab.special_id[kMask] < 0) LDDL_FAIL(-1, "vocab has no [MASK]");
  if (batch <= 0 || seq_len <= 0) return 0;
  MaskArgs M{d_input_ids, d_labels, d_special_tokens_mask, d_na, d_nb, batch, seq_len,
             mlm_probability, ignore_index, c->tab.special_id[kMask], vocab_len, {}, seed, counter,
             nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < kNumSpecial; ++k) M.special_ids[k] = c->tab.special_id[k];
  hipLaunchKernelGGL(mask_ww_kernel, dim3((unsigned)((batch + kWwWaves - 1) / kWwWaves)),
                     dim3(64 * kWwWaves), 0, as_stream(stream), M,
                     ContBits{c->d_cont_bits, c->vocab_size});
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_collate_encode_masked_ww(lddl_ctx* c, void* stream, const uint8_t* d_bytes,
                                             const int64_t* d_a_off, const int64_t* d_b_off,
                                             const int32_t* d_na, const int32_t* d_nb,
                                             int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                                             int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                             int64_t* d_labels, float mlm_probability,
                                             int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                             uint64_t counter) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (batch <= 0 || seq_len <= 0) return 0;
  if (c->tab.special_id[kCls] < 0 || c->tab.special_id[kSep] < 0 || c->tab.special_id[kMask] < 0)
    LDDL_FAIL(-1, "vocab needs [CLS], [SEP] and [MASK]");
  if (!d_input_ids || !d_token_type_ids || !d_attention_mask || !d_labels)
    LDDL_FAIL(-1, "null output");
  EncodeWwArgs E{{c->tab, d_bytes, d_a_off, d_b_off, d_na, d_nb, batch, seq_len, d_input_ids,
                  d_token_type_ids, d_attention_mask, nullptr, nullptr, nullptr, nullptr, nullptr,
                  d_labels, nullptr, ignore_index, 1,
                  MaskDraw{mlm_probability, ignore_index, c->tab.special_id[kMask], vocab_len,
                           seed, counter}},
                 ContBits{c->d_cont_bits, c->vocab_size}};
  const size_t lds = sizeof(int32_t) * 2 * (size_t)seq_len * kEncWaves;
  if (lds > 160 * 1024) LDDL_FAIL(-1, "sequence length %d too long for the collate kernel", seq_len);
  hipLaunchKernelGGL(encode_kernel<true>, dim3((unsigned)((batch + kEncWaves - 1) / kEncWaves)),
                     dim3(64 * kEncWaves), lds, as_stream(stream), E);
  LDDL_HIP(hipGetLastError());
  return 0;
}
