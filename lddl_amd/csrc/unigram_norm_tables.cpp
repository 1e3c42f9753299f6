// SentencePiece unigram, the normaliser's rules, host only: the checks of
// lddl_unigram_set_normalizer and the host images of its device tables. No HIP here.
#include <unordered_map>

#include "common.h"
#include "unigram_norm.h"

namespace lddl {

int unigram_norm_build_tables(const uint8_t* kb, const int64_t* koff, const int64_t* roff, int64_t n,
                              NormHostTables* out) {
  if (!kb || !koff || !roff || !out) LDDL_FAIL(-1, "null normaliser table");
  if (n < 1 || n > kNormMaxRules) LDDL_FAIL(-1, "n_rules %lld outside [1, 2^24]", (long long)n);
  if (koff[0] != 0 || roff[0] != 0) LDDL_FAIL(-1, "key_off and repl_off must rise from 0");
  std::unordered_map<uint32_t, uint32_t> kids;  // node << 8 | byte -> child
  std::vector<int32_t> term(1, -1);             // the rule that ends at the node
  out->rule.resize((size_t)n);
  out->max_key = out->max_repl = 0;
  for (int w = 0; w < 4; ++w) out->start[w] = out->single[w] = 0;
  out->pair.assign(1024, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = koff[i + 1] - koff[i], rlen = roff[i + 1] - roff[i];
    if (len < 1 || len > kNormMaxKey)
      LDDL_FAIL(-1, "rule %lld: a key of %lld bytes (1 to %d are allowed)", (long long)i, (long long)len, kNormMaxKey);
    if (rlen < 0 || roff[i + 1] > 0x7FFFFFFF) LDDL_FAIL(-1, "repl_off must rise from 0 and stay below 2^31");
    const uint8_t* p = kb + koff[i];
    uint32_t node = 0;
    for (int64_t k = 0; k < len; ++k) {
      const uint32_t key = node << 8 | p[k];
      auto it = kids.find(key);
      if (it == kids.end()) {
        if (term.size() >= kUniMaxNodes) LDDL_FAIL(-1, "the key trie has 2^24 nodes and more");
        it = kids.emplace(key, (uint32_t)term.size()).first;
        term.push_back(-1);
      }
      node = it->second;
    }
    if (term[node] >= 0) LDDL_FAIL(-1, "rule %lld repeats the key of rule %d", (long long)i, term[node]);
    term[node] = (int32_t)i;
    out->start[p[0] >> 6] |= 1ull << (p[0] & 63);
    if (len == 1) out->single[p[0] >> 6] |= 1ull << (p[0] & 63);
    else out->pair[(size_t)p[0] << 2 | p[1] >> 6] |= 1ull << (p[1] & 63);
    out->rule[(size_t)i] = NormRule{(uint32_t)roff[i], (uint32_t)rlen};
    if (len > out->max_key) out->max_key = (int32_t)len;
    if (rlen > out->max_repl) out->max_repl = (int32_t)rlen;
  }
  out->n_nodes = (int64_t)term.size();
  size_t slots = 16;
  while (slots < 2 * term.size()) slots <<= 1;
  out->slots.assign(slots, UniSlot{kUniEmpty, 0, -1, 0.f});
  for (int b = 0; b < 256; ++b) out->root[b] = UniSlot{kUniEmpty, 0, -1, 0.f};
  const uint32_t mask = (uint32_t)slots - 1;
  for (const auto& kv : kids) {
    if (kv.first >> 8 == 0) {
      out->root[kv.first & 255] = UniSlot{0, kv.second, term[kv.second], 0.f};
      continue;
    }
    uint32_t h = uni_hash(kv.first) & mask;
    while (out->slots[h].key != kUniEmpty) h = (h + 1) & mask;
    out->slots[h] = UniSlot{kv.first, kv.second, term[kv.second], 0.f};
  }
  return 0;
}

}  // namespace lddl
