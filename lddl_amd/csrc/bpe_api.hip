// Byte-level BPE: the lddl_bpe object, lddl_bpe_tokenize and its last stage. After
// the split (bpe_split.hip) and the merges (bpe_merge.hip) a piece is sym[x] with bit x of
// alive_bits set. Here: one device scan of the tiles' piece counts; per sentence the number of
// pieces before its first (the pre-token that holds the sentence's first byte belongs to it or
// to a later sentence: a pre-token goes to the sentence of its LAST byte); then one wave per
// tile moves its pieces to d_ids[sent_off[s] + rank in the sentence]. No host wait.
#include "arena.h"
#include "bpe.h"
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "scan.h"

struct lddl_bpe {
  int device = 0;
  lddl::BpeTables tab{};
  uint16_t* d_l1 = nullptr;
  uint8_t* d_pages = nullptr;
  lddl::BpePair* d_pairs = nullptr;
  int32_t* d_byte_id = nullptr;
  uint32_t* d_cont_bits = nullptr;
  // the pre-tokenizer (digit_group 0: GPT-2's pattern, 1 or 3: cl100k's) and the
  // whole-word table with the tokens' bytes, read only when `whole` is set
  int digit_group = 0;
  bool whole = false;
  lddl::BpeWord* d_words = nullptr;
  uint8_t* d_token_bytes = nullptr;
  int64_t* d_token_off = nullptr;
  lddl::BpeWordTable words{};
  int64_t n_tokens = 0, n_merges = 0;
  int32_t unicode[3] = {0, 0, 0};
  lddl::DevArena arena;  // the temporaries of lddl_bpe_tokenize
};

namespace lddl {
namespace {

struct TileCount {
  const uint64_t* alive;
  __device__ int64_t operator()(int64_t t) const { return __popcll(alive[t]); }
};

__device__ inline int64_t pieces_before(const BpeWork& W, int64_t x) {
  return W.tile_base[x >> 6] + __popcll(W.alive_bits[x >> 6] & ((1ull << (x & 63)) - 1));
}

// sent_base[s], s in [0, n_sent]: the pieces before the pre-token that holds byte sent_off[s]
__global__ void __launch_bounds__(256) bpe_sent_base_kernel(BpeWork W) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > W.n_sent) return;
  int64_t x = W.sent_off[s];
  x = x < 0 ? 0 : x;
  if (x >= W.n_bytes) {
    W.sent_base[s] = W.tile_base[W.n_tiles];
    return;
  }
  int64_t w = x >> 6;
  uint64_t m = bpe_upto(W.start_bits[w], (int)(x & 63));
  while (!m && w > 0) m = W.start_bits[--w];  // byte 0 starts a pre-token
  W.sent_base[s] = pieces_before(W, w * 64 + (m ? 63 - __builtin_clzll(m) : 0));
}

// the last s in [lo, n_sent) with sent_off[s] <= y (lo itself if none)
__device__ inline int64_t sent_at(const BpeWork& W, int64_t lo, int64_t y) {
  int64_t hi = W.n_sent;  // sent_off[hi] > y or hi = n_sent
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (W.sent_off[mid] <= y) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) bpe_compact_kernel(BpeWork W, int32_t max_pieces, int32_t* ids) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * 4 + wave_id();
  if (t >= W.n_tiles) return;
  const uint64_t A = W.alive_bits[t];
  if (!A) return;
  const uint64_t M = W.start_bits[t];
  // the first start past the tile, for the word that runs out of it
  // (needed iff a piece lies at or after the tile's last start): 64 mask words a step, a ballot
  // finds the first that is set; the words from n_tiles on count as all ones
  int64_t past = (t + 1) * 64;
  if (M ? (A >> (63 - __builtin_clzll(M))) != 0 : true) {
    for (int64_t w0 = t + 1;; w0 += 64) {
      const int64_t w = w0 + lane;
      const uint64_t m = w < W.n_tiles ? W.start_bits[w] : ~0ull;
      const uint64_t B = ballot(m != 0);
      if (B) {
        const int f = __builtin_ctzll(B);
        const uint32_t l32 = (uint32_t)__shfl((int)(uint32_t)m, f, 64);
        const uint32_t h32 = (uint32_t)__shfl((int)(uint32_t)(m >> 32), f, 64);
        past = (w0 + f) * 64 + __builtin_ctzll((uint64_t)h32 << 32 | l32);
        break;
      }
    }
  }
  const int64_t s_tile = sent_at(W, 0, t * 64);
  if (!((A >> lane) & 1)) return;
  const int64_t x = t * 64 + lane;
  const uint64_t hi = bpe_above(M, lane);
  const int64_t y = (hi ? t * 64 + __builtin_ctzll(hi) : past) - 1;  // the word's last byte
  int64_t s = s_tile;
  if (y - t * 64 < 256) {
    while (s + 1 < W.n_sent && W.sent_off[s + 1] <= y) ++s;
  } else {
    s = sent_at(W, s_tile, y);
  }
  const int64_t rank = pieces_before(W, x) - W.sent_base[s];
  const int64_t room = W.sent_off[s + 1] - W.sent_off[s];
  const int64_t dst = W.sent_off[s] + rank;
  if (rank >= 0 && rank < max_pieces && rank < room && dst >= 0 && dst < W.n_bytes) ids[dst] = W.sym[x];
}

__global__ void __launch_bounds__(256) bpe_sent_len_kernel(BpeWork W, int32_t max_pieces, int32_t* sent_len) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= W.n_sent) return;
  int64_t n = W.sent_base[s + 1] - W.sent_base[s];
  const int64_t room = W.sent_off[s + 1] - W.sent_off[s];
  n = n < room ? n : room;
  n = n < max_pieces ? n : max_pieces;
  sent_len[s] = (int32_t)(n > 0 ? n : 0);
}

// lddl_bpe_pretoken_stats: which pass of bpe_merge.hip a tile's pre-tokens take, by the tile
// pass's own conditions. out[0] pre-tokens, out[1] those that cross their tile's end with at
// most 64 bytes (the second window), out[2] those longer than 64 bytes (the long list).
__global__ void __launch_bounds__(256) bpe_stats_kernel(BpeWork W, unsigned long long* out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= W.n_tiles) return;
  const int64_t left = W.n_bytes - t * 64;  // bytes of the text in the tile
  if (left <= 0) return;
  const uint64_t M = left >= 64 ? W.start_bits[t] : W.start_bits[t] & ((1ull << left) - 1);
  if (!M) return;
  const uint64_t Mn = t + 1 < W.n_tiles ? W.start_bits[t + 1] : ~0ull;
  atomicAdd(out, (unsigned long long)__popcll(M));
  if (Mn & 1) return;
  const int len = Mn ? 64 - (63 - __builtin_clzll(M)) + __builtin_ctzll(Mn) : 129;
  atomicAdd(out + (len <= 64 ? 1 : 2), 1ull);
}

// the 64-bit words of temporaries the cl100k split takes on top (3 bytes a tile)
int64_t split_tmp_words(const lddl_bpe* b, int64_t n_tiles) {
  return b->digit_group ? (3 * n_tiles + 7) / 8 : 0;
}

hipError_t launch_split(const lddl_bpe* b, const BpeWork& W, int64_t clear_words, uint64_t* tmp,
                        hipStream_t st) {
  if (!b->digit_group) return bpe_launch_split(b->tab, W, clear_words, st);
  return bpe_launch_split_cl(b->tab, W, clear_words, b->digit_group, reinterpret_cast<uint8_t*>(tmp), st);
}

void release(lddl_bpe* b) {
  (void)hipFree(b->d_l1);
  (void)hipFree(b->d_pages);
  (void)hipFree(b->d_pairs);
  (void)hipFree(b->d_byte_id);
  (void)hipFree(b->d_cont_bits);
  (void)hipFree(b->d_words);
  (void)hipFree(b->d_token_bytes);
  (void)hipFree(b->d_token_off);
  delete b;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

static_assert(kBpeMaxWord == LDDL_BPE_MAX_WORD, "the header's longest exact pre-token is the kernel's");
static_assert((kBpeMaxWord & (kBpeMaxWord - 1)) == 0 && kBpeMaxWord >= 256, "a power of two >= 256");

extern "C" int lddl_bpe_create(int device, const uint8_t* class_table, int64_t class_len,
                               const uint8_t* token_bytes, const int64_t* token_off,
                               int64_t n_tokens, const int32_t* merges, int64_t n_merges,
                               lddl_bpe** out) {
  if (!out) LDDL_FAIL(-1, "null out");
  *out = nullptr;
  BpeHostTables H;
  if (bpe_build_tables(class_table, class_len, token_bytes, token_off, n_tokens, merges, n_merges, &H))
    return -1;
  LDDL_HIP(hipSetDevice(device));
  lddl_bpe* b = new lddl_bpe;
  b->device = device;
  b->n_tokens = n_tokens;
  b->n_merges = n_merges;
  for (int k = 0; k < 3; ++k) b->unicode[k] = H.unicode[k];
  int st = upload(&b->d_l1, H.l1.data(), H.l1.size() * sizeof(uint16_t));
  st = st ? st : upload(&b->d_pages, H.pages.data(), H.pages.size());
  st = st ? st : upload(&b->d_pairs, H.pairs.data(), H.pairs.size() * sizeof(BpePair));
  st = st ? st : upload(&b->d_byte_id, H.byte_id, sizeof(H.byte_id));
  st = st ? st : upload(&b->d_cont_bits, H.cont_bits.data(), H.cont_bits.size() * sizeof(uint32_t));
  st = st ? st : upload(&b->d_words, H.words.data(), H.words.size() * sizeof(BpeWord));
  st = st ? st : upload(&b->d_token_bytes, token_bytes, (size_t)token_off[n_tokens]);
  st = st ? st : upload(&b->d_token_off, token_off, ((size_t)n_tokens + 1) * sizeof(int64_t));
  if (st) {
    release(b);
    return st;
  }
  b->tab = BpeTables{b->d_l1, b->d_pages, b->d_pairs, (uint32_t)H.pairs.size() - 1, b->d_byte_id};
  b->words = BpeWordTable{b->d_words, (uint32_t)H.words.size() - 1, b->d_token_bytes, b->d_token_off};
  *out = b;
  return 0;
}

extern "C" int lddl_bpe_set_pattern(lddl_bpe* b, const char* pattern, int32_t digit_group) {
  if (!b || !pattern) LDDL_FAIL(-1, "null argument");
  const std::string p(pattern);
  if (p == "gpt2") {
    if (digit_group != 0) LDDL_FAIL(-1, "pattern gpt2 takes digit_group 0, not %d", digit_group);
  } else if (p == "cl100k") {
    if (digit_group != 1 && digit_group != 3)
      LDDL_FAIL(-1, "pattern cl100k takes digit_group 1 or 3, not %d", digit_group);
  } else {
    LDDL_FAIL(-1, "unknown pattern '%s': gpt2 or cl100k", pattern);
  }
  b->digit_group = digit_group;
  return 0;
}

extern "C" int lddl_bpe_set_whole_words(lddl_bpe* b, int32_t on) {
  if (!b) LDDL_FAIL(-1, "null bpe");
  if (on != 0 && on != 1) LDDL_FAIL(-1, "on must be 0 or 1, not %d", on);
  b->whole = on != 0;
  return 0;
}

extern "C" int lddl_bpe_destroy(lddl_bpe* b) {
  if (!b) return 0;
  (void)hipSetDevice(b->device);
  (void)hipDeviceSynchronize();
  b->arena.trim();
  release(b);
  return 0;
}

extern "C" int lddl_bpe_info(const lddl_bpe* b, int64_t* n_tokens, int64_t* n_merges,
                             int32_t* unicode_version, int32_t* max_word) {
  if (!b) LDDL_FAIL(-1, "null bpe");
  if (n_tokens) *n_tokens = b->n_tokens;
  if (n_merges) *n_merges = b->n_merges;
  if (unicode_version)
    for (int k = 0; k < 3; ++k) unicode_version[k] = b->unicode[k];
  if (max_word) *max_word = kBpeMaxWord;
  return 0;
}

extern "C" int lddl_bpe_cont_bits(const lddl_bpe* b, const uint32_t** d_bits, int64_t* n_ids) {
  if (!b || !d_bits || !n_ids) LDDL_FAIL(-1, "null argument");
  *d_bits = b->d_cont_bits;
  *n_ids = b->n_tokens;
  return 0;
}

extern "C" int lddl_bpe_tokenize(lddl_bpe* b, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                 const int64_t* d_sent_off, int64_t n_sent,
                                 const int64_t* d_doc_sent_off, int64_t n_doc, int32_t max_pieces,
                                 int32_t* d_ids, int32_t* d_sent_len) {
  if (!b) LDDL_FAIL(-1, "null bpe");
  if (n_bytes < 0 || n_sent < 0 || n_doc < 0) LDDL_FAIL(-1, "negative size");
  if (max_pieces < 1) LDDL_FAIL(-1, "max_pieces %d < 1", max_pieces);
  if (n_sent == 0) return 0;
  if ((n_bytes && !d_text) || !d_sent_off || !d_ids || !d_sent_len) LDDL_FAIL(-1, "null argument");
  hipStream_t st = as_stream(stream);
  BpeWork W{};
  W.text = d_text;
  W.n_bytes = n_bytes;
  W.n_tiles = n_bytes / 64 + 1;  // bit n_bytes exists
  W.sent_off = d_sent_off;
  W.n_sent = n_sent;
  W.doc_sent_off = d_doc_sent_off;
  W.n_doc = d_doc_sent_off ? n_doc : 0;
  W.long_cap = n_bytes / 65 + 2;
  // one block of 64-bit words: doc_bits | alive_bits | long counter (these three are cleared),
  // start_bits, tile_base, the scan's scratch, sent_base, long_list; then sym
  const int64_t nt = W.n_tiles + 1, scratch = scan_scratch_elems(W.n_tiles);
  const int64_t clear_words = 2 * nt + 1;
  const int64_t split_tmp = split_tmp_words(b, W.n_tiles);
  const int64_t words = clear_words + nt + nt + scratch + (n_sent + 1) + W.long_cap + split_tmp;
  ArenaScope tmp(&b->arena, st);
  uint64_t* base;
  if (tmp.take(&base, words)) return -100;
  if (tmp.take(&W.sym, n_bytes + 64)) return -100;
  W.doc_bits = base;
  W.alive_bits = base + nt;
  W.long_count = reinterpret_cast<unsigned long long*>(base + 2 * nt);
  W.start_bits = base + clear_words;
  W.tile_base = reinterpret_cast<int64_t*>(W.start_bits + nt);
  int64_t* scan_tmp = W.tile_base + nt;
  W.sent_base = scan_tmp + scratch;
  W.long_list = W.sent_base + n_sent + 1;
  LDDL_HIP(launch_split(b, W, clear_words, base + words - split_tmp, st));
  LDDL_HIP(bpe_launch_merge(b->tab, W, st));
  if (b->whole) LDDL_HIP(bpe_launch_whole(b->words, W, st));
  LDDL_HIP(scan_exclusive(TileCount{W.alive_bits}, W.n_tiles, W.tile_base, scan_tmp, st));
  hipLaunchKernelGGL(bpe_sent_base_kernel, dim3((unsigned)(n_sent / 256 + 1)), dim3(256), 0, st, W);
  hipLaunchKernelGGL(bpe_compact_kernel, dim3((unsigned)((W.n_tiles + 3) / 4)), dim3(256), 0, st, W,
                     max_pieces, d_ids);
  hipLaunchKernelGGL(bpe_sent_len_kernel, dim3((unsigned)((n_sent + 255) / 256)), dim3(256), 0, st, W,
                     max_pieces, d_sent_len);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_bpe_pretoken_stats(lddl_bpe* b, void* stream, const uint8_t* d_text,
                                       int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                                       const int64_t* d_doc_sent_off, int64_t n_doc,
                                       int64_t* d_stats) {
  if (!b) LDDL_FAIL(-1, "null bpe");
  if (n_bytes < 0 || n_sent < 0 || n_doc < 0) LDDL_FAIL(-1, "negative size");
  if ((n_bytes && !d_text) || !d_sent_off || !d_stats) LDDL_FAIL(-1, "null argument");
  hipStream_t st = as_stream(stream);
  BpeWork W{};
  W.text = d_text;
  W.n_bytes = n_bytes;
  W.n_tiles = n_bytes / 64 + 1;
  W.sent_off = d_sent_off;
  W.n_sent = n_sent;
  W.doc_sent_off = d_doc_sent_off;
  W.n_doc = d_doc_sent_off ? n_doc : 0;
  // doc_bits | three counters (cleared by the split's first launch) | start_bits
  const int64_t nt = W.n_tiles + 1, clear_words = nt + 3;
  ArenaScope tmp(&b->arena, st);
  uint64_t* base;
  if (tmp.take(&base, clear_words + nt + split_tmp_words(b, W.n_tiles))) return -100;
  W.doc_bits = base;
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(base + nt);
  W.start_bits = base + clear_words;
  LDDL_HIP(launch_split(b, W, clear_words, base + clear_words + nt, st));
  hipLaunchKernelGGL(bpe_stats_kernel, dim3((unsigned)((W.n_tiles + 255) / 256)), dim3(256), 0, st, W,
                     counters);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipMemcpyAsync(d_stats, counters, 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return 0;
}
