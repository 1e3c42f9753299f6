// Device helpers shared by the collate kernels (collate.hip, collate_seqpack.hip,
// collate_pairs.hip, collate_pairs_seqpack.hip): the exact vocab lookup of a whitespace-split
// string, the per-slot Philox masking decision and the whole-word ballot (the n-gram decision
// is span_dev.h's), the MODE enum, the
// slot layout of a sample (SlotLayout), the arguments of a string sample (StrSample, StrLabels)
// and the read side of a pair table (PairTable, load_id, PairSlots, scatter_labels). The
// kernels keep their loops and stores. The host side of the same units is collate_host.h.
// Each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "common.h"
#include "ctx.h"
#include "device.h"

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

// waves (= samples) per block of the collate kernels that stage a row in LDS
constexpr int kEncWaves = 4;

// what a collate kernel does on the way out: nothing (unmasked or static labels), the fused
// per-token dynamic masking, the fused whole-word one, or the fused n-gram (span) one of
// span_dev.h
enum { kPlain = 0, kFused = 1, kFusedWw = 2, kFusedSpan = 3 };

// The slots of one sample, [CLS] A [SEP] B [SEP] and padding behind: na tokens of A, end =
// na + nb + 3 slots in all. X is the caller's slot type (int32_t, or int64_t in mask_kernel).
// The layout refers to the caller's na and end, as a [&] lambda would, and does not copy them:
// with copies the compiler promotes the values in another order and the kernels' code changes
// (DESIGN §21). The string kernels and the word loops (one per kernel for whole-word and span,
// DESIGN §26) write the predicates out for the same reason.
struct SlotLayout {
  const int32_t& na;
  const int32_t& end;
  template <typename X>
  __device__ bool special(X x) const { return x == 0 || x == na + 1 || x >= end - 1; }
  template <typename X>
  __device__ bool is_sep(X x) const { return x == na + 1 || x == end - 1; }
  template <typename X>
  __device__ bool real(X x) const { return x < end; }
  template <typename X>
  __device__ int64_t segment(X x) const { return (x >= na + 2 && x < end) ? 1 : 0; }  // token type
};

// ---- the string read side (collate.hip, collate_seqpack.hip) ---------------------------------
// Two structs, not one: they sit in EncodeArgs and SeqpackArgs where their fields sat, so the
// kernels read their arguments at the offsets they had.
struct StrSample {
  Tables T;
  const uint8_t* bytes;
  const int64_t* a_off;  // [B+1] A string of sample b = bytes[a_off[b], a_off[b+1])
  const int64_t* b_off;  // [B+1]
  const int32_t* na;     // [B] token counts of A / B (host-computed, they size the batch)
  const int32_t* nb;
};
struct StrLabels {  // static masking (all nullable)
  const uint8_t* lab_bytes;
  const int64_t* lab_off;
  const uint16_t* pos;
  const int64_t* pos_off;
};

// ---- the pair-table read side (collate_pairs.hip, collate_pairs_seqpack.hip) -----------------
struct PairTable {
  const void* tokens;      // uint16 or int32 ids
  const int64_t* tok_off;  // [n_pairs + 1]
  const int32_t* len_a;
  const uint8_t* is_rn;
  // static masking (all or none)
  const uint16_t* pos;
  const void* lab;
  const int64_t* pos_off;
  const int64_t* rows;  // nullable: identity
};

template <typename ID>
__device__ inline int32_t load_id(const void* p, int64_t i) {
  return (int32_t) reinterpret_cast<const ID*>(p)[i];
}

// The id of slot x before masking, of the pair whose tokens start at t0. Like SlotLayout it
// refers to the caller's values, as a [&] lambda would.
template <typename ID>
struct PairSlots {
  const PairTable& P;
  const int64_t& t0;
  const SlotLayout& lay;
  const int32_t& cls;
  const int32_t& sep;
  __device__ int32_t operator()(int32_t x) const {
    if (x == 0) return cls;
    if (lay.is_sep(x)) return sep;
    if (x >= lay.end) return 0;
    return load_id<ID>(P.tokens, t0 + x - (x <= lay.na ? 1 : 2));
  }
};

// slab[0, limit) = the static label of pair q's slot or -1, one wave; a position >= limit is
// dropped
template <typename ID>
__device__ inline void scatter_labels(const PairTable& P, int64_t q, int32_t* slab, int32_t limit,
                                      int lane) {
  for (int32_t x = lane; x < limit; x += 64) slab[x] = -1;
  wave_sync();
  const int64_t p0 = P.pos_off[q];
  const int32_t npos = (int32_t)(P.pos_off[q + 1] - p0);
  for (int32_t k = lane; k < npos; k += 64) {
    const int32_t p = P.pos[p0 + k];
    if (p < limit) slab[p] = load_id<ID>(P.lab, p0 + k);
  }
  wave_sync();
}

}  // namespace
}  // namespace lddl
