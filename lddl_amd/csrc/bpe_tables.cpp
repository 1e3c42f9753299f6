// Byte-level BPE, host only: the checks of lddl_bpe_create and the host images of
// the device tables. No HIP here, so a CPU program can call it.
#include "bpe.h"

#include <cstring>

#include "common.h"

namespace lddl {

int bpe_build_tables(const uint8_t* ct, int64_t ct_len, const uint8_t* tb, const int64_t* off,
                     int64_t n_tokens, const int32_t* merges, int64_t n_merges,
                     BpeHostTables* out) {
  if (!ct || !tb || !off || (n_merges > 0 && !merges) || !out) LDDL_FAIL(-1, "null bpe table");
  // ---- the class table (tools/bpe_classes.py) ----
  uint32_t fmt = 0, n_l1 = 0, n_pages = 0;
  if (ct_len >= 32) {
    memcpy(&fmt, ct + 4, 4);
    memcpy(&n_l1, ct + 12, 4);
    memcpy(&n_pages, ct + 16, 4);
  }
  if (ct_len < 32 || memcmp(ct, "LBPC", 4) || fmt != 1 || n_l1 != (0x110000u >> 8) ||
      n_pages == 0 || n_pages > 65535 || ct_len != 32 + 2 * (int64_t)n_l1 + 64 * (int64_t)n_pages)
    LDDL_FAIL(-1, "class table: not a bpe_classes.bin of format 1");
  out->l1.resize(n_l1);
  memcpy(out->l1.data(), ct + 32, 2 * (size_t)n_l1);
  for (uint16_t p : out->l1)
    if (p >= n_pages) LDDL_FAIL(-1, "class table: page index %u of %u", p, n_pages);
  out->pages.assign(ct + 32 + 2 * (size_t)n_l1, ct + ct_len);
  for (int k = 0; k < 3; ++k) out->unicode[k] = ct[8 + k];

  // ---- the tokens ----
  if (n_tokens < 256 || n_tokens > (int64_t)1 << 30) LDDL_FAIL(-1, "n_tokens %lld outside [256, 2^30]", (long long)n_tokens);
  if (n_merges < 0 || n_merges >= (int64_t)kBpeMaxRank)
    LDDL_FAIL(-1, "%lld merges: the ABI takes ranks below 2^26", (long long)n_merges);
  for (int64_t i = 0; i < n_tokens; ++i)
    if (off[i + 1] < off[i] || off[0] != 0) LDDL_FAIL(-1, "token_off must rise from 0");
  for (int b = 0; b < 256; ++b) out->byte_id[b] = -1;
  std::vector<uint8_t> known((size_t)n_tokens, 0);  // a base token or the result of a line so far
  for (int64_t i = 0; i < n_tokens; ++i)
    if (off[i + 1] - off[i] == 1 && out->byte_id[tb[off[i]]] < 0) {
      out->byte_id[tb[off[i]]] = (int32_t)i;
      known[(size_t)i] = 1;
    }
  for (int b = 0; b < 256; ++b)
    if (out->byte_id[b] < 0) LDDL_FAIL(-1, "the vocabulary has no token for the single byte 0x%02x", b);

  // ---- the whole-word table (ignore_merges): every token of 2 .. kBpeMaxWord bytes by the
  // hash of its bytes; of tokens with equal bytes the lowest id ----
  size_t n_words = 0, wslots = 16;
  for (int64_t i = 0; i < n_tokens; ++i) n_words += off[i + 1] - off[i] >= 2 && off[i + 1] - off[i] <= kBpeMaxWord;
  while (wslots < 2 * n_words) wslots <<= 1;
  out->words.assign(wslots, BpeWord{0, kBpeEmpty, 0});
  for (int64_t i = 0; i < n_tokens; ++i) {
    const int64_t len = off[i + 1] - off[i];
    if (len < 2 || len > kBpeMaxWord) continue;
    uint64_t h = 0;
    for (int64_t k = 0; k < len; ++k) h = h * kBpeWordP + tb[off[i] + k] + 1;
    size_t s = bpe_word_slot(h) & (wslots - 1);
    for (; out->words[s].id != kBpeEmpty; s = (s + 1) & (wslots - 1)) {
      const BpeWord& e = out->words[s];
      if (e.hash == h && e.len == (uint32_t)len && !memcmp(tb + off[e.id], tb + off[i], (size_t)len)) break;
    }
    if (out->words[s].id == kBpeEmpty) out->words[s] = BpeWord{h, (uint32_t)i, (uint32_t)len};
  }

  // ---- the merges, in rank order ----
  size_t slots = 16;
  while (slots < 2 * (size_t)n_merges) slots <<= 1;
  out->pairs.assign(slots, BpePair{kBpeEmpty, 0, 0, 0});
  const uint32_t mask = (uint32_t)slots - 1;
  for (int64_t r = 0; r < n_merges; ++r) {
    const int64_t l = merges[3 * r], rt = merges[3 * r + 1], m = merges[3 * r + 2];
    if (l < 0 || l >= n_tokens || rt < 0 || rt >= n_tokens || m < 0 || m >= n_tokens)
      LDDL_FAIL(-1, "merge %lld: id outside the vocabulary", (long long)r);
    if (!known[(size_t)l] || !known[(size_t)rt])
      LDDL_FAIL(-1, "merge %lld: operand %lld is neither a base token nor the result of an earlier line",
                (long long)r, (long long)(known[(size_t)l] ? rt : l));
    const int64_t ll = off[l + 1] - off[l], rl = off[rt + 1] - off[rt];
    if (off[m + 1] - off[m] != ll + rl || memcmp(tb + off[m], tb + off[l], (size_t)ll) ||
        memcmp(tb + off[m] + ll, tb + off[rt], (size_t)rl))
      LDDL_FAIL(-1, "merge %lld: the bytes of token %lld are not those of %lld + %lld", (long long)r,
                (long long)m, (long long)l, (long long)rt);
    uint32_t h = bpe_pair_hash((uint32_t)l, (uint32_t)rt) & mask;
    for (; out->pairs[h].left != kBpeEmpty; h = (h + 1) & mask)
      if (out->pairs[h].left == (uint32_t)l && out->pairs[h].right == (uint32_t)rt)
        LDDL_FAIL(-1, "merge %lld repeats the pair of merge %u", (long long)r, out->pairs[h].rank);
    out->pairs[h] = BpePair{(uint32_t)l, (uint32_t)rt, (uint32_t)r, (uint32_t)m};
    known[(size_t)m] = 1;
  }

  // ---- fairseq's is_beginning_of_word, negated: a reachable token that does not open with a
  // space continues a word; special tokens (never reached from bytes) count as beginnings ----
  out->cont_bits.assign(((size_t)n_tokens + 31) / 32, 0u);
  for (int64_t i = 0; i < n_tokens; ++i)
    if (known[(size_t)i] && tb[off[i]] != 0x20) out->cont_bits[(size_t)i >> 5] |= 1u << (i & 31);
  return 0;
}

}  // namespace lddl
