// Device code that more than one tokenizer unit uses (unit map: tokenize.hip): the code-point
// table and UTF-8, literal special tokens, a word in registers (B32) and its vocab probes, the
// Bloom-filtered greedy WordPiece step (piece_step / wordpiece32), and a pre-tokenizer unit's
// normalised word (unit_word, norm_regs).
// Everything is in an anonymous namespace, as collate_dev.h has it and as these functions were
// when the kernels shared one file: each unit gets its own internal copy, nothing is emitted for
// a function a unit does not use, and the compiler's inlining decisions in the streaming kernel
// are those it made before (`inline` would give wordpiece32 and the other plain functions
// linkonce_odr linkage, which the inliner weighs differently).
#pragma once
#include <cstdint>

#include "ctx.h"
#include "device.h"

namespace lddl {
namespace {

__device__ inline uint32_t tab_entry(const Tables& T, uint32_t cp) {
  if (cp > 0x10FFFF) return kDrop << 30;
  return T.pages[(uint32_t)T.l1[cp >> 8] * 256u + (cp & 255u)];
}

__device__ inline uint32_t utf8_next(const uint8_t* b, int64_t end, int64_t& i) {
  const uint32_t c = b[i];
  if (c < 0x80) { ++i; return c; }
  const int len = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
  if (len == 1 || i + len > end) { ++i; return 0xFFFD; }
  uint32_t cp = c & (0x7Fu >> len);
  for (int k = 1; k < len; ++k) {
    const uint32_t d = b[i + k];
    if ((d & 0xC0) != 0x80) { ++i; return 0xFFFD; }
    cp = (cp << 6) | (d & 0x3F);
  }
  i += len;
  return cp;
}

__device__ inline int put_utf8(uint8_t* o, uint32_t cp) {
  if (cp < 0x80) { o[0] = (uint8_t)cp; return 1; }
  if (cp < 0x800) { o[0] = 0xC0 | (cp >> 6); o[1] = 0x80 | (cp & 63); return 2; }
  if (cp < 0x10000) {
    o[0] = 0xE0 | (cp >> 12); o[1] = 0x80 | ((cp >> 6) & 63); o[2] = 0x80 | (cp & 63);
    return 3;
  }
  o[0] = 0xF0 | (cp >> 18); o[1] = 0x80 | ((cp >> 12) & 63); o[2] = 0x80 | ((cp >> 6) & 63);
  o[3] = 0x80 | (cp & 63);
  return 4;
}

__device__ inline bool match_special(const uint8_t* b, int64_t i, int64_t end, int k) {
  // "[PAD]" "[UNK]" "[CLS]" "[SEP]" "[MASK]"
  const char* s = k == 0 ? "[PAD]" : k == 1 ? "[UNK]" : k == 2 ? "[CLS]" : k == 3 ? "[SEP]" : "[MASK]";
  const int L = k == 4 ? 6 : 5;
  if (i + L > end) return false;
  for (int j = 1; j < L; ++j)
    if (b[i + j] != (uint8_t)s[j]) return false;
  return true;
}

constexpr int kPcs = 8;    // pieces per unit held per lane (more -> fallback)
constexpr int kNorm = 32;  // normalised bytes per unit on the generic path (more -> fallback)

// unit categories per byte position
enum : uint32_t { kCatRun = 0, kCatSep = 1, kCatIso = 2, kCatSpecial = 3 };

__device__ inline int match_special_at(const Tables& T, const uint8_t* b, int64_t i, int64_t end) {
  for (int k = 0; k < kNumSpecial; ++k)
    if (T.special_id[k] >= 0 && match_special(b, i, end, k)) return k;
  return -1;
}

// Up to 32 bytes of a word as four little-endian 64-bit words (bytes past the word: don't care,
// every use masks by length).
struct B32 {
  uint64_t w0, w1, w2, w3;
};

// bytes [s, 32) moved to the front (s in 0..31)
__device__ inline B32 shr_bytes(const B32& v, int s) {
  const int q = s >> 3, r = (s & 7) * 8;
  uint64_t a0 = q == 0 ? v.w0 : q == 1 ? v.w1 : q == 2 ? v.w2 : v.w3;
  uint64_t a1 = q == 0 ? v.w1 : q == 1 ? v.w2 : q == 2 ? v.w3 : 0ull;
  uint64_t a2 = q == 0 ? v.w2 : q == 1 ? v.w3 : 0ull;
  uint64_t a3 = q == 0 ? v.w3 : 0ull;
  if (r) {
    a0 = (a0 >> r) | (a1 << (64 - r));
    a1 = (a1 >> r) | (a2 << (64 - r));
    a2 = (a2 >> r) | (a3 << (64 - r));
    a3 >>= r;
  }
  return B32{a0, a1, a2, a3};
}

// The pieces of one unit: the lane's column of an LDS buffer (lane l's piece q at b[64 q]).
struct Pcs {
  int32_t* b;
  __device__ void put(int n, int32_t v) { b[64 * n] = v; }
  __device__ int32_t get(int q) const { return b[64 * q]; }
};

// Diagnostic build: work counters of phase B (per lane; summed at the kernel's end).
[[maybe_unused]] constexpr int kTokCounters = 12;  // 10: kQSlow lanes of the passes, 11: passes with at least one
struct TokStats {
#ifdef LDDL_STAMPS
  uint64_t c[kTokCounters];
  __device__ void add(int i, uint64_t v) { c[i] += v; }
  // once per wave-level iteration: only the first active lane counts
  __device__ void wave(int i) {
    const uint64_t m = __builtin_amdgcn_ballot_w64(true);
    if ((uint32_t)__lane_id() == (uint32_t)__builtin_ctzll(m)) c[i] += 1;
  }
#else
  __device__ void add(int, uint64_t) {}
  __device__ void wave(int) {}
#endif
};

// Bytes 8 .. len-1 (len 13..32) of a against piece id's zero-padded 32-byte copy (the hash key
// already matched bytes 0..11).
__device__ inline bool tail_match(const Tables& T, int32_t id, const B32& a, int len) {
  const ulonglong2* p = reinterpret_cast<const ulonglong2*>(T.vlong + 4 * (int64_t)id);
  const ulonglong2 lo = p[0], hi = p[1];
  const uint64_t d = keep_bytes(lo.y ^ a.w1, len - 8) | keep_bytes(hi.x ^ a.w2, len - 16) |
                     keep_bytes(hi.y ^ a.w3, len - 24);
  return d == 0;
}

// Vocab probe of the first `len` (1..32) bytes of a: exact key for <= 12 bytes (k0 = bytes 0..7,
// k1 = bytes 8..11), longer pieces confirmed against their 32-byte copies.

// probe32 split in two, so that several probes' first table loads are in flight together:
// probe_first computes the key and issues the load of the home slot, probe_finish examines it
// and walks the collision chain (rarely more than the home slot).
struct Probe {
  uint64_t k0;
  uint32_t k1, want, slot;
  VEnt e;
};
__device__ inline Probe probe_first(const Tables& T, const B32& a, int len, uint32_t cont) {
  Probe q;
  q.k0 = keep_bytes(a.w0, len);
  q.k1 = (uint32_t)keep_bytes(a.w1, len - 8 < 4 ? len - 8 : 4);
  q.want = kMetaValid | (cont ? kMetaCont : 0u) | (len > 12 ? kMetaLong : 0u) | ((uint32_t)len << 21);
  q.slot = (uint32_t)vhash(q.k0, q.k1, len, cont) & T.vmask;
  q.e = T.vhash[q.slot];
  return q;
}
__device__ inline int32_t probe_finish(const Tables& T, const B32& a, int len, Probe q) {
  for (;;) {
    if (!(q.e.meta & kMetaValid)) return -1;
    if (q.e.k0 == q.k0 && q.e.k1 == q.k1 && (q.e.meta & ~0x1FFFFFu) == q.want &&
        (len <= 12 || tail_match(T, meta_id(q.e.meta), a, len)))
      return meta_id(q.e.meta);
    q.slot = (q.slot + 1) & T.vmask;
    q.e = T.vhash[q.slot];
  }
}

// Bloom candidates for the pieces starting at a's first byte: bit L-1 set iff the filter may
// contain (cont, bytes[0, L)), L = 1 .. maxl (<= 32). (Round 5 read the filter words of 2 / 4 / 8
// lengths before testing any: 19.31 / 21.1 / 22.9 ms per 2 GB against 19.32, the grouped reads
// cost registers; profiles/r05i_tok_variants.txt, code on branch ab/tok-cp-variants.)
__device__ inline uint32_t bloom_candidates32(const uint32_t* bloom, const B32& a, int maxl,
                                              uint32_t cont, TokStats* ts = nullptr) {
  uint32_t h = 0, cand = 0;
#pragma unroll
  for (int L = 1; L <= 32; ++L) {
    // wave-uniform exit (lanes past their own maxl compute don't-care bits, masked below): no
    // exec-mask bookkeeping per length
    if (!ballot(L <= maxl)) break;
    if (ts) {
      ts->wave(4);
      ts->add(5, L <= maxl);
    }
    const uint64_t wv = L <= 8 ? a.w0 : L <= 16 ? a.w1 : L <= 24 ? a.w2 : a.w3;
    const uint32_t byte = (uint32_t)(wv >> (8 * ((L - 1) & 7))) & 0xFFu;
    h = h * kBloomP + byte + 1u;
    const uint32_t x = bloom_mix(h, (uint32_t)L, cont);
    const uint32_t msk = bloom_bits(x);
    cand |= (bloom[bloom_word(x)] & msk) == msk ? 1u << (L - 1) : 0u;
  }
  return maxl >= 32 ? cand : cand & ((1u << maxl) - 1u);
}

// One greedy longest-match step of a word held in registers: the longest vocab piece (continuation
// iff start > 0) starting at byte `start`; returns its id and length, or -1 (no piece matches:
// the word is [UNK]). Per step, the Bloom filter (LDS) gives the lengths that may be pieces (every
// vocab piece is in it: the longest candidate that hits is the greedy match), and the two longest
// candidates' home slots are loaded together, so a lane waits on ONE table round trip per piece
// in the common case. first_probe_missed: phase A already probed the whole word (start 0).
__device__ inline int32_t piece_step(const Tables& T, const uint32_t* bloom, const B32& v, int nb,
                                     uint64_t ends, int start, bool first_probe_missed, int& out_len,
                                     TokStats* ts = nullptr) {
  const B32 a = shr_bytes(v, start);
  const uint32_t cont = start > 0;
  const uint64_t e = ends >> start;  // bit L: a piece of length L may end here
  int len = nb - start < T.max_piece_bytes ? nb - start : T.max_piece_bytes;
  {  // the longest length <= len that ends on a character boundary (bit L-1 of okl: length L)
    const uint64_t okl = (e >> 1) & ((1ull << len) - 1ull);
    len = okl ? 64 - __clzll(okl) : 0;
  }
  uint32_t cand = len > 0 ? bloom_candidates32(bloom, a, len, cont, ts) & (uint32_t)(e >> 1) : 0u;
  // (the caller may already know that the whole word is not one piece)
  if (first_probe_missed && start == 0 && len == nb) cand &= ~(1u << (len - 1));
  int32_t id = -1;
  while (cand) {
    if (ts) {
      ts->wave(6);
      ts->add(7, 1);
    }
    const int l1 = 32 - __clz(cand);
    const uint32_t r1 = cand & ~(1u << (l1 - 1));
    const int l2 = r1 ? 32 - __clz(r1) : 0;
    const Probe q1 = probe_first(T, a, l1, cont);
    const Probe q2 = probe_first(T, a, l2 ? l2 : l1, cont);
    id = probe_finish(T, a, l1, q1);
    if (id >= 0) {
      len = l1;
      break;
    }
    if (l2) {
      id = probe_finish(T, a, l2, q2);
      if (id >= 0) {
        len = l2;
        break;
      }
    }
    cand = l2 ? r1 & ~(1u << (l2 - 1)) : 0u;
  }
  out_len = len;
  return id;
}

// Greedy longest-match WordPiece (HF WordPiece::tokenize) of a normalised word of nb <= 32 bytes
// held in registers. ends: bit e set iff a piece may end at byte e (a UTF-8 character boundary;
// all bits for ASCII). Returns the piece count written to pc, or -1 if more than kPcs pieces.
// (Round 3 probed the full length alone first, then two candidates per round trip: 21.9 ms per
// 2 GiB against 20.7 now; three candidates per trip spilled VGPRs and took 22.1 ms, r04o.)
__device__ int wordpiece32(const Tables& T, const uint32_t* bloom, const B32& v, int nb,
                           uint64_t ends, Pcs& pc, bool first_probe_missed = false,
                           TokStats* ts = nullptr) {
  int n = 0, start = 0;
  while (start < nb) {
    if (ts) {
      ts->wave(2);
      ts->add(3, 1);
    }
    int len;
    const int32_t id = piece_step(T, bloom, v, nb, ends, start, first_probe_missed, len, ts);
    if (id < 0) {  // no piece: the whole word is [UNK]
      pc.put(0, T.special_id[kUnk]);
      return 1;
    }
    if (n == kPcs) return -1;
    pc.put(n++, id);
    start += len;
  }
  return n;
}

// 32 bytes of text from byte `start` (unaligned); bytes at or past `n_bytes` read as 0 and are
// never loaded.
__device__ inline B32 load32(const uint8_t* __restrict__ text, int64_t n_bytes, int64_t start) {
  const int64_t a = start & ~(int64_t)3;
  const int r = (int)(start & 3);
  uint32_t d[9];
  if (a + 36 <= n_bytes) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(text + a);
#pragma unroll
    for (int k = 0; k < 9; ++k) d[k] = p[k];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      uint32_t v = 0;
      for (int q = 0; q < 4; ++q)
        if (a + 4 * k + q < n_bytes) v |= (uint32_t)text[a + 4 * k + q] << (8 * q);
      d[k] = v;
    }
  }
  uint32_t o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], r);
  return B32{(uint64_t)o[0] | ((uint64_t)o[1] << 32), (uint64_t)o[2] | ((uint64_t)o[3] << 32),
             (uint64_t)o[4] | ((uint64_t)o[5] << 32), (uint64_t)o[6] | ((uint64_t)o[7] << 32)};
}

__device__ inline uint64_t swar_lower(uint64_t v) {  // A-Z -> a-z on ASCII bytes
  const uint64_t k3f = 0x3f3f3f3f3f3f3f3full, k25 = 0x2525252525252525ull,
                 k80 = 0x8080808080808080ull;
  return v | ((((v + k3f) & ~(v + k25)) & k80) >> 2);
}

// ---------------------------------------------------------------------------------------------
// Non-ASCII ("slow") units from registers. unit_word's loop pays one dependent global load per
// raw byte and three more per non-ASCII code point (UTF-8 tail, l1, pages) while the other lanes
// of the phase-B pass wait: 45 % of phase B in the lookup launch
// (profiles/r09_tok_phaseB_split_parent.txt). norm_regs takes a unit of <= 32 raw bytes
// with one load32, decodes its non-ASCII code points from the registers (at most kSlowCps; more:
// the loop), loads their l1 and pages entries with nothing else between, and only then walks the
// bytes (ASCII through s_ascii in LDS; no global load in the walk but a kMulti entry's pool
// bytes), writing the normalised word to the lane's LDS row as the loop does. Same rules as
// utf8_next / unit_word's loop, byte for byte.
// ---------------------------------------------------------------------------------------------
constexpr int kSlowCps = 4;
constexpr uint64_t k80 = 0x8080808080808080ull;

__device__ inline uint32_t byte_at(const B32& v, int j) {  // j in 0..31
  const uint64_t w = j < 8 ? v.w0 : j < 16 ? v.w1 : j < 24 ? v.w2 : v.w3;
  return (uint32_t)(w >> (8 * (j & 7))) & 0xFFu;
}

// bit i of the result: bit 7 of byte i of t (t has no other bits set). The product's terms
// never share a bit position, so nothing carries.
__device__ inline uint32_t top_bits(uint64_t t) {
  return (uint32_t)(((t >> 7) * 0x0102040810204080ull) >> 56);
}
__device__ inline uint32_t top_bits32(const B32& t) {
  return top_bits(t.w0) | top_bits(t.w1) << 8 | top_bits(t.w2) << 16 | top_bits(t.w3) << 24;
}

// utf8_next over raw bytes held in registers (end <= 32)
__device__ inline uint32_t utf8_next_regs(const B32& v, int end, int& i) {
  const uint32_t c = byte_at(v, i);
  if (c < 0x80) { ++i; return c; }
  const int len = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
  if (len == 1 || i + len > end) { ++i; return 0xFFFD; }
  uint32_t cp = c & (0x7Fu >> len);
  for (int k = 1; k < len; ++k) {
    const uint32_t d = byte_at(v, i + k);
    if ((d & 0xC0) != 0x80) { ++i; return 0xFFFD; }
    cp = (cp << 6) | (d & 0x3F);
  }
  i += len;
  return cp;
}

// Returns the normalised bytes written to w, -1: more than kNorm, -2: more than kSlowCps non-ASCII
// code points (nothing done).
__device__ __forceinline__ int norm_regs(const Tables& T, const uint32_t* s_ascii, const uint8_t* __restrict__ text,
                         int64_t n_bytes, int64_t start, int len, uint8_t* w) {
  const B32 raw = load32(text, n_bytes, start);
  const uint32_t in_unit = len >= 32 ? ~0u : (1u << len) - 1u;
  // bit j: raw byte j is not ASCII. The walk below meets such a byte only where a code point
  // starts (a lead, a lone continuation, 0xFF), in the order in which they are decoded here.
  const uint32_t hi = top_bits32(B32{raw.w0 & k80, raw.w1 & k80, raw.w2 & k80, raw.w3 & k80}) & in_unit;
  uint32_t cp[kSlowCps], ent[kSlowCps], advs = 0, rest = hi;
#pragma unroll
  for (int k = 0; k < kSlowCps; ++k) {
    cp[k] = 0;
    if (rest) {
      const int j = __builtin_ctz(rest);
      int i = j;
      cp[k] = utf8_next_regs(raw, len, i);
      advs |= (uint32_t)(i - j) << (3 * k);
      rest = i >= 32 ? 0u : rest & (~0u << i);
    }
  }
  if (rest) return -2;
  // the table entries of the decoded code points: two dependent loads each, before the walk
#pragma unroll
  for (int k = 0; k < kSlowCps; ++k) {
    ent[k] = 0;
    if (advs >> (3 * k)) ent[k] = tab_entry(T, cp[k]);
  }
  int nb = 0;
  for (int j = 0; j < len;) {
    uint32_t c, e;
    if (!((hi >> j) & 1u)) {
      c = byte_at(raw, j);
      e = s_ascii[c];
      ++j;
    } else {  // the next decoded code point
      c = cp[0];
      e = ent[0];
      j += (int)(advs & 7u);
      advs >>= 3;
#pragma unroll
      for (int k = 0; k + 1 < kSlowCps; ++k) cp[k] = cp[k + 1], ent[k] = ent[k + 1];
    }
    if ((e >> 30) == kDrop) continue;
    if (!(e & kIdent) && (e & kMulti)) {  // (rare: the pool bytes are loaded one after another)
      const uint8_t* p = T.pool + (e & 0xFFFFFFu);
      const int olen = p[0];
      if (nb + olen > kNorm) return -1;
      for (int q = 0; q < olen; ++q) w[nb + q] = p[2 + q];
      nb += olen;
    } else {
      const uint32_t o = (e & kIdent) ? c : e & 0x1FFFFFu;
      const int olen = o < 0x80 ? 1 : o < 0x800 ? 2 : o < 0x10000 ? 3 : 4;
      if (nb + olen > kNorm) return -1;
      put_utf8(w + nb, o);
      nb += olen;
    }
  }
  return nb;
}

// The normalised word of a word / isolated-char unit in registers (<= 32 bytes) and the byte
// positions where a piece may end. status: 0 ok, 1 empty (every char dropped: 0 pieces), -1 the
// unit needs the lane kernel (> kNorm normalised bytes). ASCII units are loaded straight from the
// text (SWAR lowercase); others are normalised through the lane's LDS row `w` first, from
// registers where norm_regs takes the unit and `regs` allows it, else byte by byte from the text.
struct UnitWord {
  B32 v;
  int nb;
  uint64_t ends;
  int status;
};

__device__ __forceinline__ UnitWord unit_word(const Tables& T, const uint32_t* s_ascii, const uint8_t* __restrict__ text,
                              int64_t n_bytes, int64_t start, int len, bool unit_slow, uint8_t* w,
                              bool regs) {
  UnitWord u;
  u.status = 0;
  if (!unit_slow && len <= 32 && T.ascii_mode != 0) {
    B32 v = load32(text, n_bytes, start);
    if (T.ascii_mode == 1) v = B32{swar_lower(v.w0), swar_lower(v.w1), swar_lower(v.w2), swar_lower(v.w3)};
    u.v = v;
    u.nb = len;
    u.ends = ~0ull;
    return u;
  }
  int nb = -2;
  if (regs && len <= 32 && T.ascii_mode != 0) nb = norm_regs(T, s_ascii, text, n_bytes, start, len, w);
  if (nb == -2) {  // byte by byte from the text
    nb = 0;
    int64_t j = start;
    const int64_t je = start + len;
    while (j < je) {
      const uint32_t b0 = text[j];
      uint32_t cp, e;
      if (b0 < 0x80) {
        cp = b0;
        e = s_ascii[b0];
        ++j;
      } else {
        cp = utf8_next(text, je, j);
        e = tab_entry(T, cp);
      }
      if ((e >> 30) == kDrop) continue;
      uint8_t ob[12];
      int olen;
      if (e & kIdent) olen = put_utf8(ob, cp);
      else if (e & kMulti) {
        const uint8_t* p = T.pool + (e & 0xFFFFFFu);
        olen = p[0];
        for (int q = 0; q < olen; ++q) ob[q] = p[2 + q];
      } else olen = put_utf8(ob, e & 0x1FFFFFu);
      if (nb + olen > kNorm) {
        nb = -1;
        break;
      }
      for (int q = 0; q < olen; ++q) w[nb + q] = ob[q];
      nb += olen;
    }
  }
  u.nb = nb;
  if (nb <= 0) {
    u.status = nb < 0 ? -1 : 1;
    return u;
  }
  const uint64_t* w8 = reinterpret_cast<const uint64_t*>(w);
  u.v = B32{w8[0], w8[1], w8[2], w8[3]};
  // a piece may end before every byte that does not continue a character (10xxxxxx), and at nb
  const uint32_t cont = top_bits32(B32{u.v.w0 & ~(u.v.w0 << 1) & k80, u.v.w1 & ~(u.v.w1 << 1) & k80,
                                       u.v.w2 & ~(u.v.w2 << 1) & k80, u.v.w3 & ~(u.v.w3 << 1) & k80});
  u.ends = ((uint64_t)(~cont & ~1u) & ((1ull << nb) - 1ull)) | 1ull << nb;
  return u;
}

}  // namespace
}  // namespace lddl
