// SentencePiece unigram: the tables of an lddl_unigram and the device-side pieces
// the three kernel units share (unigram_match.hip, unigram_viterbi.hip, unigram_api.hip).
// unigram_tables.cpp builds the host images; it sees this header without the device parts.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif
#include <cstdint>
#include <vector>

namespace lddl {

constexpr int kUniMaxWord = 1024;  // LDDL_UNIGRAM_MAX_WORD
constexpr int kUniMaxNest = 16;    // LDDL_UNIGRAM_MAX_NEST
constexpr int kUniAsciiWs = 1;     // LDDL_UNIGRAM_ASCII_WS
constexpr int64_t kUniMaxPieces = 1 << 20;  // an edge packs id | end << 20
constexpr uint32_t kUniMaxNodes = 1u << 24;  // a key packs node << 8 | byte
constexpr uint32_t kUniEmpty = 0xFFFFFFFFu;  // `key` of a free slot
constexpr float kUniMaxScore = 1e30f;  // |score| above it is refused: path sums stay finite
enum { kUniNormal = 1, kUniUnknown = 2, kUniControl = 3, kUniUser = 4, kUniUnused = 5, kUniByte = 6 };

// One edge of the byte trie, (node, byte) -> child: a slot of the open-addressing table (linear
// probing, key = node << 8 | byte) or of the root's direct table (key = 0 where the edge exists).
struct alignas(16) UniSlot {
  uint32_t key, child;
  int32_t id;   // the piece that ends at `child`, or -1
  float score;  // that piece's
};

inline
#ifdef __HIP__
    __host__ __device__
#endif
    uint32_t
    uni_hash(uint32_t key) {
  uint32_t h = (key >> 8) * 0x9E3779B1u ^ (key & 255u) * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  return h ^ (h >> 13);
}

// What unigram_tables.cpp makes of the arguments of lddl_unigram_create.
struct UniHostTables {
  std::vector<UniSlot> slots;  // a power of two, at least twice the nodes
  UniSlot root[256];
  uint32_t pre_node = 0;  // the node of E2 96 81
  int32_t pre_id = -1;    // the piece that is E2 96 81 alone
  float pre_score = 0.f;  // and its score
  float unk_score = 0.f;  // min NORMAL score - 10
  int64_t n_nodes = 0;
  std::vector<uint32_t> cont_bits;  // bit id: a matchable piece that does not start with E2 96 81
};
// 0, or -1 with the message set (common.h)
int unigram_build_tables(const uint8_t* piece_bytes, const int64_t* piece_off, const float* scores,
                         const int32_t* types, int64_t n_pieces, int32_t unk_id, UniHostTables* out);

// Kernel-side view of the tables (passed by value).
struct UniTables {
  const UniSlot* slots;
  const UniSlot* root;
  uint32_t mask, pre_node;
  int32_t pre_id, unk_id;
  float unk_score, pre_score;
  int32_t ascii_ws;
};

// One tokenize call's text and temporaries. A tile is 64 bytes; n_tiles covers n_bytes + 1.
struct UniWork {
  const uint8_t* text;
  int64_t n_bytes, n_tiles;
  const int64_t* sent_off;
  int64_t n_sent;
  uint64_t* sent_bits;   // bit x: a sentence starts at byte x
  uint64_t* start_bits;  // bit x: a word starts at byte x
  uint64_t* break_bits;  // bit x: byte x is a space, a sentence start or past the text
  uint64_t* alive_bits;  // bit x: a piece starts at byte x
  uint64_t* pre_bits;    // bit x: the piece E2 96 81 alone stands before the piece at byte x
  int32_t* sym;          // sym[x]: the id of the piece at byte x
  int64_t* long_list;    // the starts of the words longer than 64 bytes
  int64_t long_cap;
  unsigned long long* long_count;
  int64_t* tile_base;  // pieces before tile t
  int64_t* sent_base;  // pieces before sentence s's first byte
};

#ifdef __HIP__
// unigram_match.hip: clears `clear_words` 64-bit words from sent_bits (sent_bits, alive_bits,
// pre_bits and the long counter are one region), marks the sentence starts, writes start_bits
// and break_bits.
hipError_t unigram_launch_words(const UniTables& T, const UniWork& W, int64_t clear_words, hipStream_t st);
// unigram_match.hip: the tile pass (match and Viterbi of every word of at most 64 bytes).
hipError_t unigram_launch_tiles(const UniTables& T, const UniWork& W, hipStream_t st);
// unigram_viterbi.hip: the long list.
hipError_t unigram_launch_long(const UniTables& T, const UniWork& W, hipStream_t st);

__device__ inline uint64_t uni_upto(uint64_t m, int j) { return m & ((2ull << j) - 1); }
__device__ inline uint64_t uni_above(uint64_t m, int j) { return m & ~((2ull << j) - 1); }

__device__ inline bool uni_space(const UniTables& T, uint32_t b) {
  return b == 0x20 || (T.ascii_ws && (b == 0x09 || b == 0x0A || b == 0x0C || b == 0x0D));
}

__device__ inline void uni_or_bits(uint64_t* bits, int64_t first, uint64_t m) {
  if (!m) return;
  const int sh = (int)(first & 63);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(bits + (first >> 6));
  if (m << sh) atomicOr(w, m << sh);
  if (sh && (m >> (64 - sh))) atomicOr(w + 1, m >> (64 - sh));
}

// The character of byte p of a word b[lo, hi): 0 if p is a continuation byte that a whole
// sequence claims, else the character's length: what its lead byte announces if all of it lies
// in the word, else 1 (a stray continuation byte, a truncated character, C0, C1, F5-FF).
__device__ inline int uni_lead_len(uint32_t c) {
  return (c >= 0xC2 && c <= 0xDF) ? 2 : (c >= 0xE0 && c <= 0xEF) ? 3 : (c >= 0xF0 && c <= 0xF4) ? 4 : 1;
}
__device__ inline int uni_whole_len(const uint8_t* b, int q, int hi) {
  const int n = uni_lead_len(b[q]);
  if (q + n > hi) return 1;
  for (int k = 1; k < n; ++k)
    if ((b[q + k] & 0xC0) != 0x80) return 1;
  return n;
}
__device__ inline int uni_char_len(const uint8_t* b, int p, int lo, int hi) {
  if ((b[p] & 0xC0) == 0x80) {
    for (int k = 1; k <= 3 && p - k >= lo; ++k) {
      if (b[p - k] >= 0xC0) return uni_whole_len(b, p - k, hi) > k ? 0 : 1;
      if (b[p - k] < 0x80) break;
    }
    return 1;
  }
  return uni_whole_len(b, p, hi);
}

// one step of the trie: the edge (node, byte), false on a miss
__device__ inline bool uni_step(const UniTables& T, uint32_t node, uint32_t byte, UniSlot* e) {
  if (node == 0) {
    *e = T.root[byte];
    return e->key != kUniEmpty;
  }
  const uint32_t key = node << 8 | byte;
  for (uint32_t h = uni_hash(key) & T.mask;; h = (h + 1) & T.mask) {
    const uint4 v = *reinterpret_cast<const uint4*>(T.slots + h);
    if (v.x == kUniEmpty) return false;
    if (v.x == key) {
      e->key = v.x;
      e->child = v.y;
      e->id = (int32_t)v.z;
      e->score = __uint_as_float(v.w);
      return true;
    }
  }
}

// The walk of one lane from `node` along b[pos, hi): every prefix that is a piece is appended to
// the lane's row of the edge table as (id | end << 20, score bits); edge k of row r is
// edge[k * stride + r], so that the lanes of a round write side by side. Returns the count;
// *one is set if a piece ended `clen` bytes after the start.
__device__ inline int uni_walk(const UniTables& T, const uint8_t* b, uint32_t node, int pos, int hi,
                               uint2* edge, int stride, int row, int clen, bool* one) {
  int cnt = 0;
  const int p0 = pos;
  UniSlot e;
  while (pos < hi && uni_step(T, node, b[pos], &e)) {
    node = e.child;
    ++pos;
    if (e.id >= 0 && cnt < kUniMaxNest) {
      edge[cnt * stride + row] = make_uint2((uint32_t)e.id | (uint32_t)pos << 20, __float_as_uint(e.score));
      ++cnt;
      if (pos - p0 == clen) *one = true;
    }
  }
  return cnt;
}

// best[j] / back[j]: the best score of a path that ends behind byte j, and its last piece as
// id | (start + 1) << 20 (0: it starts at the prefix). Strictly greater replaces.
__device__ inline void uni_relax(float* best, uint32_t* back, int j, float cand, uint32_t piece) {
  if (cand > best[j]) {
    best[j] = cand;
    back[j] = piece;
  }
}

// the edges of row `row` from a start of score bs; piece = the start's code << 20
__device__ inline void uni_relax_row(const uint2* edge, int stride, int row, int n, float bs,
                                     uint32_t start_code, float* best, uint32_t* back) {
  for (int k = 0; k < n; ++k) {
    const uint2 e = edge[k * stride + row];
    uni_relax(best, back, (int)(e.x >> 20) - 1, bs + __uint_as_float(e.y), (e.x & 0xFFFFFu) | start_code << 20);
  }
}
#endif

}  // namespace lddl
