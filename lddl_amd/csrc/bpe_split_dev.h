// Byte-level BPE, what the two pre-tokenizers share on the device (bpe_split.hip: GPT-2's pattern,
// bpe_split_cl.hip: cl100k's): the code byte of a text position and the step to the character
// before it. A code is class | len << 2 | flags; len 0 is a continuation byte that a lead claims.
#pragma once
#include "bpe.h"

namespace lddl {

constexpr uint8_t kOutside = 0x80, kDocStart = 0x20;  // code: class | len << 2 | flags

__device__ inline int bpe_class(const BpeTables& T, uint32_t cp) {
  if (cp >= 0x110000u) return kBpeOther;
  const uint32_t page = T.l1[cp >> 8];
  return (T.pages[page * 64 + ((cp & 255) >> 2)] >> (2 * (cp & 3))) & 3;
}

// the code of position x (see the head comment of bpe_split.hip); reads the text and the
// document bits only
__device__ inline uint8_t char_code(const BpeTables& T, const BpeWork& W, int64_t x) {
  if (x < 0 || x >= W.n_bytes) return kOutside;
  const uint8_t* t = W.text;
  const uint32_t b = t[x];
  const bool ds = x == 0 || bpe_bit(W.doc_bits, x);
  const uint8_t flags = ds ? kDocStart : 0;
  // the length a lead byte announces and whether the sequence from q is whole
  auto whole = [&](int64_t q, int* len) {
    const uint32_t c = t[q];
    const int n = c < 0x80 ? 1 : (c >= 0xC2 && c <= 0xDF) ? 2 : (c >= 0xE0 && c <= 0xEF) ? 3
                  : (c >= 0xF0 && c <= 0xF4) ? 4 : 0;
    *len = n;
    if (n == 0 || q + n > W.n_bytes) return false;
    for (int k = 1; k < n; ++k)
      if ((t[q + k] & 0xC0) != 0x80 || bpe_bit(W.doc_bits, q + k)) return false;
    return true;
  };
  int n;
  if ((b & 0xC0) == 0x80) {  // a continuation byte: claimed by a whole sequence up to 3 back?
    if (!ds)
      for (int k = 1; k <= 3 && x - k >= 0; ++k)
        if (t[x - k] >= 0xC0) {
          if (whole(x - k, &n) && n > k) return flags;  // length 0
          break;
        }
    return flags | (1 << 2) | kBpeOther;
  }
  if (!whole(x, &n)) return flags | (1 << 2) | kBpeOther;
  uint32_t cp = b;
  if (n == 2) cp = (b & 0x1F) << 6 | (t[x + 1] & 0x3F);
  if (n == 3) cp = (b & 0x0F) << 12 | (t[x + 1] & 0x3F) << 6 | (t[x + 2] & 0x3F);
  if (n == 4) cp = (b & 0x07) << 18 | (t[x + 1] & 0x3F) << 12 | (t[x + 2] & 0x3F) << 6 | (t[x + 3] & 0x3F);
  return flags | (uint8_t)(n << 2) | (uint8_t)bpe_class(T, cp);
}

constexpr int kNone = 4;  // the class of "no character"

// class of the character before window index i (kNone at a document start), and whether it is
// U+0020; i's own code is not outside
__device__ inline int prev_class(const uint8_t* code, const uint8_t* byte, int i, bool* is20) {
  *is20 = false;
  if (code[i] & kDocStart) return kNone;
  int k = 1;
  while (k < 4 && ((code[i - k] >> 2) & 7) == 0) ++k;  // skip claimed continuation bytes
  if (code[i - k] & kOutside) return kNone;
  *is20 = byte[i - k] == 0x20;
  return code[i - k] & 3;
}

}  // namespace lddl
