// Byte-level BPE: the tables of an lddl_bpe and the device-side views the three
// kernel units share (bpe_split.hip, bpe_merge.hip, bpe_api.hip). bpe_tables.cpp builds the host
// images; it sees this header without the device parts.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif
#include <cstdint>
#include <string>
#include <vector>

namespace lddl {

constexpr int kBpeMaxWord = 1024;  // LDDL_BPE_MAX_WORD
constexpr uint32_t kBpeNoRank = 0xFFFFFFFFu;
constexpr uint32_t kBpeMaxRank = 1u << 26;
constexpr uint32_t kBpeEmpty = 0xFFFFFFFFu;  // `left` of a free slot of the pair table
enum { kBpeOther = 0, kBpeLetter = 1, kBpeNumber = 2, kBpeSpace = 3 };

// One slot of the open-addressing table (left, right) -> (rank, merged); linear probing.
struct alignas(16) BpePair {
  uint32_t left, right, rank, merged;
};

inline
#ifdef __HIP__
    __host__ __device__
#endif
    uint32_t
    bpe_pair_hash(uint32_t left, uint32_t right) {
  uint32_t h = left * 0x9E3779B1u ^ right * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  return h ^ (h >> 13);
}

// One slot of the whole-word table (ignore_merges): the polynomial hash of a token's
// bytes (h = h * kBpeWordP + byte + 1 mod 2^64, so one prefix scan hashes every word of a tile)
// -> the token; linear probing; id kBpeEmpty: a free slot. The bytes are token_off's.
struct alignas(16) BpeWord {
  uint64_t hash;
  uint32_t id, len;
};
constexpr uint64_t kBpeWordP = 0x9E3779B97F4A7C15ull;

inline
#ifdef __HIP__
    __host__ __device__
#endif
    uint32_t
    bpe_word_slot(uint64_t h) {  // the product's high half: the low bits of a polynomial mod 2^64 mix badly
  return (uint32_t)(((h ^ (h >> 29)) * 0xBF58476D1CE4E5B9ull) >> 32);
}

// What bpe_tables.cpp makes of the arguments of lddl_bpe_create.
struct BpeHostTables {
  std::vector<BpeWord> words;  // tokens of 2 .. kBpeMaxWord bytes; a power of two, at most half full
  std::vector<BpePair> pairs;  // a power of two of slots, at most half of them taken
  int32_t byte_id[256];
  std::vector<uint32_t> cont_bits;  // bit id: the token's bytes do not start with 0x20
  std::vector<uint16_t> l1;         // the class table (tools/bpe_classes.py)
  std::vector<uint8_t> pages;
  int32_t unicode[3];
};
// 0, or -1 with the message set (common.h)
int bpe_build_tables(const uint8_t* class_table, int64_t class_len, const uint8_t* token_bytes,
                     const int64_t* token_off, int64_t n_tokens, const int32_t* merges,
                     int64_t n_merges, BpeHostTables* out);

// Kernel-side view of the tables (passed by value).
struct BpeTables {
  const uint16_t* l1;
  const uint8_t* pages;
  const BpePair* pairs;
  uint32_t pair_mask;
  const int32_t* byte_id;
};

// One tokenize call's text and temporaries. A tile is 64 bytes; n_tiles covers n_bytes + 1.
struct BpeWork {
  const uint8_t* text;
  int64_t n_bytes, n_tiles;
  const int64_t* sent_off;
  int64_t n_sent;
  const int64_t* doc_sent_off;  // NULL: every sentence is a document
  int64_t n_doc;
  uint64_t* doc_bits;    // bit x: a document starts at byte x
  uint64_t* start_bits;  // bit x: a pre-token starts at byte x (every x >= n_bytes too)
  uint64_t* alive_bits;  // bit x: a piece starts at byte x
  int32_t* sym;          // sym[x]: that piece's id
  int64_t* long_list;    // the starts of the pre-tokens longer than 64 bytes
  int64_t long_cap;
  unsigned long long* long_count;
  int64_t* tile_base;  // pieces before tile t (a scan of the alive bits)
  int64_t* sent_base;  // pieces before sentence s's first
};

// Kernel-side view of the whole-word table and of the tokens' bytes.
struct BpeWordTable {
  const BpeWord* slots;
  uint32_t mask;
  const uint8_t* bytes;
  const int64_t* off;
};

#ifdef __HIP__
// bpe_split.hip: clears doc_bits, alive_bits and the long counter (one region, `clear_words`
// 64-bit words from doc_bits), marks the document starts, writes start_bits.
hipError_t bpe_launch_split(const BpeTables& T, const BpeWork& W, int64_t clear_words, hipStream_t st);
// its first two launches alone (the clear and the document starts)
hipError_t bpe_launch_docs(const BpeWork& W, int64_t clear_words, hipStream_t st);
// bpe_split_cl.hip: bpe_launch_split for the cl100k pattern with digit groups of 1 or 3;
// run_tmp: 3 * n_tiles bytes (a tile's run summaries, then its carries)
hipError_t bpe_launch_split_cl(const BpeTables& T, const BpeWork& W, int64_t clear_words,
                               int digit_group, uint8_t* run_tmp, hipStream_t st);
// bpe_whole.hip, after the merges: a pre-token whose bytes are a token becomes that token
hipError_t bpe_launch_whole(const BpeWordTable& V, const BpeWork& W, hipStream_t st);
// bpe_merge.hip: sym and alive_bits from text and start_bits (the tile pass, then the long list).
hipError_t bpe_launch_merge(const BpeTables& T, const BpeWork& W, hipStream_t st);

__device__ inline bool bpe_bit(const uint64_t* bits, int64_t x) { return (bits[x >> 6] >> (x & 63)) & 1; }
// bits of m at or below lane j / strictly above it (j in 0 .. 63)
__device__ inline uint64_t bpe_upto(uint64_t m, int j) { return m & ((2ull << j) - 1); }
__device__ inline uint64_t bpe_above(uint64_t m, int j) { return m & ~((2ull << j) - 1); }
#endif

}  // namespace lddl
