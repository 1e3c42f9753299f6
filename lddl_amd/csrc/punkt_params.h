// The two blobs of lddl_punkt_set_params (punkt.hip) on the host: the character class table is
// validated in place, the parameter records are parsed into the open-addressing table the
// segmenter's lookup probes. PkEnt and the hash are the one definition host and device share.
// (Host-only and free of the HIP runtime, like plan_split.h, so a CPU program can test it:
// tests/punkt_params_check.cpp.)
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.h"

#ifdef __HIPCC__
#define LDDL_HD __host__ __device__
#else
#define LDDL_HD
#endif

namespace lddl {

enum : uint32_t { kKAbbrev = 1, kKStarter = 2, kKOrtho = 3, kKColloc = 4 };
constexpr int kMaxKey = 255;  // longest parameter key (bytes)

struct PkEnt {  // open-addressing entry; kind 0 = empty
  uint32_t h;
  uint32_t off;  // key bytes in keys[]
  uint16_t la, lb;
  uint8_t kind, value;
  uint16_t pad;
};

LDDL_HD inline uint32_t fnv_step(uint32_t h, uint32_t b) { return (h ^ b) * 0x01000193u; }
LDDL_HD inline uint32_t key_hash(uint32_t h, uint32_t kind) {
  h ^= kind * 0x9E3779B9u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  return h;
}

// value of the key (kind, a, b) in the table (hash, hmask, keys), -1: absent. b counts for
// collocations only. (The hash is written out here and in the parser: as a function of its own,
// inlined or not, it changes segment_eval_kernel<true>'s instruction stream.)
LDDL_HD inline int find_param(const PkEnt* hash, uint32_t hmask, const uint8_t* keys, uint32_t kind,
                              const uint8_t* a, int la, const uint8_t* b, int lb) {
  uint32_t h = 0x811C9DC5u;
  for (int k = 0; k < la; ++k) h = fnv_step(h, a[k]);
  if (kind == kKColloc) {
    h = fnv_step(h, 0x100u);
    for (int k = 0; k < lb; ++k) h = fnv_step(h, b[k]);
  }
  h = key_hash(h, kind);
  for (uint32_t p = h & hmask;; p = (p + 1) & hmask) {
    const PkEnt en = hash[p];
    if (en.kind == 0) return -1;
    if (en.h != h || en.kind != kind || en.la != la || (kind == kKColloc && en.lb != lb)) continue;
    bool eq = true;
    for (int k = 0; k < la && eq; ++k) eq = keys[en.off + k] == a[k];
    for (int k = 0; kind == kKColloc && k < lb && eq; ++k) eq = keys[en.off + la + k] == b[k];
    if (eq) return en.value;
  }
}

// The class table blob: "LDPK", u32 version, pages, lower pairs; u16 l1[0x1100]; u8 pages[][256];
// i32 (cp, lower) pairs, little-endian. The pointers lie inside the caller's blob.
constexpr int64_t kPunktL1Bytes = 0x1100 * 2;
struct PunktClassBlob {
  const uint8_t *l1, *pages, *lower;
  uint32_t n_pages, n_lower;
};
inline uint32_t le32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

inline int parse_punkt_table(const uint8_t* table, int64_t table_bytes, PunktClassBlob* out) {
  if (!table || table_bytes < 16 + kPunktL1Bytes || memcmp(table, "LDPK", 4) != 0)
    LDDL_FAIL(-1, "bad Punkt character table");
  const uint32_t n_pages = le32(table + 8), n_lower = le32(table + 12);
  const int64_t need = 16 + kPunktL1Bytes + (int64_t)n_pages * 256 + (int64_t)n_lower * 8;
  if (le32(table + 4) != 1 || table_bytes < need) LDDL_FAIL(-1, "truncated Punkt character table");
  const uint8_t *l1 = table + 16, *pages = l1 + kPunktL1Bytes, *lower = pages + (int64_t)n_pages * 256;
  for (int i = 0; i < 0x1100; ++i)  // the device indexes pages[] with l1[cp >> 8] unchecked
    if ((uint32_t)(l1[2 * i] | l1[2 * i + 1] << 8) >= n_pages)
      LDDL_FAIL(-1, "Punkt character table: l1[%d] names a page past the last of %u", i, n_pages);
  for (uint32_t i = 1; i < n_lower; ++i)  // lower_cp bisects the pairs by code point
    if (le32(lower + 8 * (int64_t)i) <= le32(lower + 8 * (int64_t)(i - 1)))
      LDDL_FAIL(-1, "Punkt character table: lowercase pairs not ascending at %u", i);
  *out = PunktClassBlob{l1, pages, lower, n_pages, n_lower};
  return 0;
}

// The parameter records as the device table: hash[hmask + 1] entries over keys[].
struct PunktParamTable {
  std::vector<PkEnt> hash;
  std::vector<uint8_t> keys;
  uint32_t hmask = 0;
  int32_t n_ent = 0;  // distinct (kind, a, b)
};

// records: u8 kind, u8 value, u16 la, u16 lb, a bytes, b bytes. A set: of equal keys the first
// record wins (ortho_context keys are unique in nltk).
inline int parse_punkt_records(const uint8_t* records, int64_t records_bytes, PunktParamTable* out) {
  if (!records && records_bytes > 0) LDDL_FAIL(-1, "null Punkt parameter records");
  std::vector<PkEnt> ents;
  PunktParamTable t;
  for (int64_t r = 0; r < records_bytes;) {
    if (r + 6 > records_bytes) LDDL_FAIL(-1, "truncated Punkt parameter record");
    const uint8_t* q = records + r;
    PkEnt e{};
    e.kind = q[0];
    e.value = q[1];
    e.la = (uint16_t)(q[2] | (q[3] << 8));
    e.lb = (uint16_t)(q[4] | (q[5] << 8));
    if (e.kind < kKAbbrev || e.kind > kKColloc) LDDL_FAIL(-1, "bad Punkt parameter kind %d", e.kind);
    if (e.la > kMaxKey || e.lb > kMaxKey)
      LDDL_FAIL(-1, "Punkt parameter key longer than %d bytes", kMaxKey);
    if (r + 6 + e.la + e.lb > records_bytes) LDDL_FAIL(-1, "truncated Punkt parameter record");
    uint32_t h = 0x811C9DC5u;
    for (int k = 0; k < e.la; ++k) h = fnv_step(h, q[6 + k]);
    if (e.kind == kKColloc) {
      h = fnv_step(h, 0x100u);
      for (int k = 0; k < e.lb; ++k) h = fnv_step(h, q[6 + e.la + k]);
    }
    e.h = key_hash(h, e.kind);
    e.off = (uint32_t)t.keys.size();
    t.keys.insert(t.keys.end(), q + 6, q + 6 + e.la + e.lb);
    ents.push_back(e);
    r += 6 + e.la + e.lb;
  }
  uint32_t cap = 16;
  while (cap < 2 * ents.size() + 16) cap <<= 1;
  t.hash.assign(cap, PkEnt{});
  t.hmask = cap - 1;
  for (const PkEnt& e : ents) {
    uint32_t p = e.h & t.hmask;
    bool dup = false;
    while (t.hash[p].kind && !dup) {
      const PkEnt& o = t.hash[p];
      dup = o.h == e.h && o.kind == e.kind && o.la == e.la && o.lb == e.lb &&
            (e.la + e.lb == 0 || !memcmp(t.keys.data() + o.off, t.keys.data() + e.off, e.la + e.lb));
      if (!dup) p = (p + 1) & t.hmask;
    }
    if (!dup) t.hash[p] = e;
    t.n_ent += !dup;
  }
  *out = std::move(t);
  return 0;
}

}  // namespace lddl
