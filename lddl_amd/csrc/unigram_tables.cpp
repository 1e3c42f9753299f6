// SentencePiece unigram, host only: the checks of lddl_unigram_create and the host
// images of the device tables. No HIP here, so a CPU program can call it.
#include "unigram.h"

#include <cmath>
#include <cstring>
#include <unordered_map>

#include "common.h"

namespace lddl {

int unigram_build_tables(const uint8_t* pb, const int64_t* off, const float* scores,
                         const int32_t* types, int64_t n, int32_t unk_id, UniHostTables* out) {
  if (!pb || !off || !scores || !types || !out) LDDL_FAIL(-1, "null unigram table");
  if (n < 1 || n > kUniMaxPieces) LDDL_FAIL(-1, "n_pieces %lld outside [1, 2^20]", (long long)n);
  if (off[0] != 0) LDDL_FAIL(-1, "piece_off must rise from 0");
  for (int64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) LDDL_FAIL(-1, "piece_off must rise from 0");
  if (unk_id < 0 || unk_id >= n) LDDL_FAIL(-1, "unk_id %d outside the vocabulary", unk_id);
  int64_t n_unk = 0;
  float min_score = INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(scores[i]) || std::fabs(scores[i]) > kUniMaxScore)
      LDDL_FAIL(-1, "piece %lld: the score is not finite (or beyond 1e30)", (long long)i);
    n_unk += types[i] == kUniUnknown;
    if (types[i] == kUniNormal && scores[i] < min_score) min_score = scores[i];
  }
  if (types[unk_id] != kUniUnknown || n_unk != 1)
    LDDL_FAIL(-1, "unk_id %d is not the one UNKNOWN piece (%lld have that type)", unk_id, (long long)n_unk);
  if (min_score == INFINITY) LDDL_FAIL(-1, "no NORMAL piece");
  out->unk_score = min_score - 10.0f;

  // ---- the byte trie of the NORMAL and USER_DEFINED pieces; node 0 is the root ----
  std::unordered_map<uint32_t, uint32_t> kids;  // node << 8 | byte -> child
  std::vector<uint32_t> parent(1, 0);
  std::vector<int32_t> term(1, -1);  // the piece that ends at the node
  static const uint8_t kPre[3] = {0xE2, 0x96, 0x81};
  for (int64_t i = 0; i < n; ++i) {
    if (types[i] != kUniNormal && types[i] != kUniUser) continue;
    const uint8_t* p = pb + off[i];
    const int64_t len = off[i + 1] - off[i];
    if (len == 0) LDDL_FAIL(-1, "piece %lld is empty", (long long)i);
    for (int64_t k = 1; k + 3 <= len; ++k)
      if (!memcmp(p + k, kPre, 3))
        LDDL_FAIL(-1, "piece %lld has the space mark E2 96 81 at an interior position", (long long)i);
    uint32_t node = 0;
    for (int64_t k = 0; k < len; ++k) {
      const uint32_t key = node << 8 | p[k];
      auto it = kids.find(key);
      if (it == kids.end()) {
        if (parent.size() >= kUniMaxNodes) LDDL_FAIL(-1, "the trie has 2^24 nodes and more");
        it = kids.emplace(key, (uint32_t)parent.size()).first;
        parent.push_back(node);
        term.push_back(-1);
      }
      node = it->second;
    }
    if (term[node] >= 0) LDDL_FAIL(-1, "piece %lld repeats piece %d", (long long)i, term[node]);
    term[node] = (int32_t)i;
  }
  // a child's index is above its parent's: one rising pass counts the pieces on each path
  std::vector<uint8_t> nest(parent.size(), 0);
  for (size_t v = 1; v < parent.size(); ++v) {
    const int d = nest[parent[v]] + (term[v] >= 0);
    if (d > kUniMaxNest)
      LDDL_FAIL(-1, "piece %d is the 17th on its path from the root: more than %d nested pieces", term[v], kUniMaxNest);
    nest[v] = (uint8_t)d;
  }
  uint32_t node = 0;
  for (int k = 0; k < 3; ++k) {
    auto it = kids.find(node << 8 | kPre[k]);
    node = it == kids.end() ? 0 : it->second;
    if (!node) break;
  }
  if (!node || term[node] < 0) LDDL_FAIL(-1, "no piece is the space mark E2 96 81 alone");
  out->pre_node = node;
  out->pre_id = term[node];
  out->pre_score = scores[term[node]];
  out->n_nodes = (int64_t)parent.size();

  size_t slots = 16;
  while (slots < 2 * parent.size()) slots <<= 1;
  out->slots.assign(slots, UniSlot{kUniEmpty, 0, -1, 0.f});
  for (int b = 0; b < 256; ++b) out->root[b] = UniSlot{kUniEmpty, 0, -1, 0.f};
  const uint32_t mask = (uint32_t)slots - 1;
  for (const auto& kv : kids) {
    const int32_t id = term[kv.second];
    const UniSlot s{kv.first, kv.second, id, id >= 0 ? scores[id] : 0.f};
    if (kv.first >> 8 == 0) {
      out->root[kv.first & 255] = UniSlot{0, s.child, s.id, s.score};
      continue;
    }
    uint32_t h = uni_hash(kv.first) & mask;
    while (out->slots[h].key != kUniEmpty) h = (h + 1) & mask;
    out->slots[h] = s;
  }

  out->cont_bits.assign(((size_t)n + 31) / 32, 0u);
  for (int64_t i = 0; i < n; ++i)
    if ((types[i] == kUniNormal || types[i] == kUniUser) &&
        (off[i + 1] - off[i] < 3 || memcmp(pb + off[i], kPre, 3)))
      out->cont_bits[(size_t)i >> 5] |= 1u << (i & 31);
  return 0;
}

}  // namespace lddl
