// SentencePiece unigram, the normaliser and byte fallback: the lddl_unigram object,
// the rule tables of lddl_unigram_set_normalizer and what the kernel units share
// (unigram_norm.hip, unigram_bytes.hip, unigram_norm_api.hip, unigram_api.hip).
// unigram_norm_tables.cpp sees this header without the device parts.
#pragma once
#include <memory>

#include "unigram.h"

namespace lddl {

// LDDL_UNIGRAM_NORM_MAX_KEY: a key spans two tiles at most, and a clean tile entered at up to 60
// leaves as if entered at its head, so no key makes every tile wait for the one before
constexpr int kNormMaxKey = 61;
constexpr int64_t kNormMaxRules = 1 << 24;
constexpr int32_t kNormCopy = -1, kNormBad = -2;  // a lane's rule: the character as it stands / U+FFFD
struct NormRule {
  uint32_t off, len;  // the replacement: blob[off, off + len)
};

// What unigram_norm_tables.cpp makes of the arguments of lddl_unigram_set_normalizer: the keys
// as a byte trie in the slot layout of the pieces' trie (UniSlot.id = the rule that ends there).
struct NormHostTables {
  std::vector<UniSlot> slots;
  UniSlot root[256];
  uint64_t start[4];            // bit b: some key starts with byte b
  uint64_t single[4];           // bit b: byte b alone is a key
  std::vector<uint64_t> pair;   // 1,024 words; bit b0 << 8 | b1: a longer key starts with b0 b1
  std::vector<NormRule> rule;
  int32_t max_key = 0, max_repl = 0;
  int64_t n_nodes = 0;
};
// 0, or -1 with the message set
int unigram_norm_build_tables(const uint8_t* key_blob, const int64_t* key_off, const int64_t* repl_off,
                              int64_t n_rules, NormHostTables* out);

// Kernel-side view (passed by value).
struct NormTables {
  const UniSlot* slots;
  const UniSlot* root;
  const NormRule* rule;
  const uint8_t* repl;
  const uint64_t* pair;
  uint64_t start[4], single[4];
  uint32_t mask;
  int32_t max_key;
};

// One normalize call. A tile is 64 bytes of the input, n_tiles = ceil(n_bytes / 64).
// info[t]: bits 0-7 the tile's exit (the bytes of the next tile that a character or key which
// starts here takes), bits 8-15 the largest entry up to which that exit holds, bits 16-17 `head`
// (the leading continuation bytes no character of the tile claims), bit 31 "cleanish": no byte
// starts a key and every byte behind `head` belongs to a well-formed character of its sentence.
struct NormWork {
  const uint8_t* text;
  int64_t n_bytes, n_tiles;
  const int64_t* sent_off;
  int64_t n_sent;
  uint64_t* sent_bits;  // bit x: a sentence starts at byte x; n_tiles + 2 words
  uint32_t* info;
  uint8_t* entry;       // the tile's first live byte
  int32_t* count;       // its output bytes
  int64_t* tile_base;   // the output bytes before it; [n_tiles] the total
};
constexpr uint32_t kNormCleanish = 1u << 31;

#ifdef __HIP__
// unigram_norm.hip. plan: sent_bits, info, entry, count, tile_base (scan_tmp: scan_scratch_elems
// of n_tiles) and out_sent_off; write: out_text from the same NormWork.
hipError_t unigram_norm_launch_plan(const NormTables& N, const NormWork& W, int64_t* scan_tmp,
                                    int64_t* out_sent_off, hipStream_t st);
hipError_t unigram_norm_launch_write(const NormTables& N, const NormWork& W, uint8_t* out_text,
                                     int64_t out_cap, hipStream_t st);
// d_stats[2]: the plan's tiles, those on the dirty path
hipError_t unigram_norm_launch_stats(const NormWork& W, int64_t* d_stats, hipStream_t st);
// unigram_bytes.hip: byte fallback on the finished paths (cover: n_tiles words of scratch).
hipError_t unigram_launch_bytes(const UniTables& T, const UniWork& W, const int32_t* byte_ids,
                                uint64_t* cover, hipStream_t st);
#endif

}  // namespace lddl

#ifdef __HIP__
#include "arena.h"

struct lddl_unigram {
  int device = 0;
  lddl::UniTables tab{};
  lddl::UniSlot* d_slots = nullptr;
  lddl::UniSlot* d_root = nullptr;
  uint32_t* d_cont_bits = nullptr;
  int64_t n_pieces = 0, n_nodes = 0, n_slots = 0;
  lddl::DevArena arena;  // the temporaries of lddl_unigram_tokenize
  // ---- §33 ----
  std::vector<uint32_t> cont_host;  // d_cont_bits as lddl_unigram_create made it
  int32_t* d_byte_ids = nullptr;    // [256], or null: byte fallback is off
  lddl::NormTables norm{};          // norm.rule == nullptr: the normaliser is off
  lddl::UniSlot* d_nslots = nullptr;
  lddl::UniSlot* d_nroot = nullptr;
  lddl::NormRule* d_nrule = nullptr;
  uint8_t* d_nrepl = nullptr;
  uint64_t* d_npair = nullptr;
  int64_t n_rules = 0;
  int32_t max_repl = 0;
  // the plan lddl_unigram_normalize_write reads: lddl_unigram_normalize_plan's temporaries
  std::unique_ptr<lddl::ArenaScope> plan;
  lddl::NormWork plan_work{};
  hipStream_t plan_stream = nullptr;
  int64_t* h_total = nullptr;    // pinned: the planned size, valid once plan_done has passed
  hipEvent_t plan_done = nullptr;
};
namespace lddl {
// unigram_norm_api.hip: frees the rule tables (the normaliser is off afterwards)
void unigram_norm_free(lddl_unigram* u);
}  // namespace lddl
#endif
