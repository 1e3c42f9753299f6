// SentencePiece unigram: the lddl_unigram object, lddl_unigram_tokenize and its last
// stage. After the words (unigram_match.hip), the tile pass and the long pass
// (unigram_viterbi.hip) a piece is sym[x] with bit x of alive_bits set, and bit x of pre_bits
// says that the prefix piece stands alone before it: that piece has no byte of its own, so the
// counts are of pieces, not of bytes. Here: one device scan of the tiles' piece counts; per
// sentence the pieces before its first byte (a word never crosses a sentence start); then one
// wave per tile moves its pieces to d_ids[sent_off[s] + rank in the sentence]. No host wait.
#include "arena.h"
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "scan.h"
#include "unigram_norm.h"

namespace lddl {
namespace {

struct TileCount {
  const uint64_t* alive;
  const uint64_t* pre;
  __device__ int64_t operator()(int64_t t) const { return __popcll(alive[t]) + __popcll(pre[t]); }
};

// the pieces before byte x; the prefix piece that stands before x itself is not among them
__device__ inline int64_t pieces_before(const UniWork& W, int64_t x) {
  const uint64_t below = (1ull << (x & 63)) - 1;
  return W.tile_base[x >> 6] + __popcll(W.alive_bits[x >> 6] & below) + __popcll(W.pre_bits[x >> 6] & below);
}

__global__ void __launch_bounds__(256) uni_sent_base_kernel(UniWork W) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > W.n_sent) return;
  int64_t x = W.sent_off[s];
  x = x < 0 ? 0 : x;
  W.sent_base[s] = x >= W.n_bytes ? W.tile_base[W.n_tiles] : pieces_before(W, x);
}

// the last s in [lo, n_sent) with sent_off[s] <= y (lo itself if none)
__device__ inline int64_t sent_at(const UniWork& W, int64_t lo, int64_t y) {
  int64_t hi = W.n_sent;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (W.sent_off[mid] <= y) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) uni_compact_kernel(UniWork W, int32_t pre_id, int32_t max_pieces,
                                                          int32_t* ids) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * 4 + wave_id();
  if (t >= W.n_tiles) return;
  const uint64_t A = W.alive_bits[t];
  if (!A) return;
  const int64_t s_tile = sent_at(W, 0, t * 64);
  if (!((A >> lane) & 1)) return;
  const int64_t x = t * 64 + lane;
  int64_t s = s_tile;
  while (s + 1 < W.n_sent && W.sent_off[s + 1] <= x) ++s;  // at most 64 steps past empty ones
  const bool pre = (W.pre_bits[t] >> lane) & 1;
  const int64_t room = W.sent_off[s + 1] - W.sent_off[s];
  int64_t rank = pieces_before(W, x) - W.sent_base[s];
  for (int k = pre ? 0 : 1; k < 2; ++k, ++rank) {
    const int64_t dst = W.sent_off[s] + rank;
    if (rank >= 0 && rank < max_pieces && rank < room && dst >= 0 && dst < W.n_bytes)
      ids[dst] = k == 0 ? pre_id : W.sym[x];
  }
}

__global__ void __launch_bounds__(256) uni_sent_len_kernel(UniWork W, int32_t max_pieces, int32_t* sent_len) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= W.n_sent) return;
  int64_t n = W.sent_base[s + 1] - W.sent_base[s];
  const int64_t room = W.sent_off[s + 1] - W.sent_off[s];
  n = n < room ? n : room;
  n = n < max_pieces ? n : max_pieces;
  sent_len[s] = (int32_t)(n > 0 ? n : 0);
}

// lddl_unigram_word_stats: which pass a tile's words take, by the tile pass's own conditions.
// out[0] words, out[1] those that cross their tile's end with at most 64 bytes (the second
// window), out[2] those longer than 64 bytes (the long list).
__global__ void __launch_bounds__(256) uni_stats_kernel(UniWork W, unsigned long long* out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= W.n_tiles) return;
  const uint64_t S = W.start_bits[t];
  if (!S) return;
  atomicAdd(out, (unsigned long long)__popcll(S));
  const uint64_t Bn = t + 1 < W.n_tiles ? W.break_bits[t + 1] : ~0ull;
  const int js = 63 - __builtin_clzll(S);
  if (uni_above(W.break_bits[t], js) || (Bn & 1)) return;
  const int len = Bn ? 64 - js + __builtin_ctzll(Bn) : 129;
  atomicAdd(out + (len <= 64 ? 1 : 2), 1ull);
}

void release(lddl_unigram* u) {
  u->plan.reset();
  unigram_norm_free(u);
  (void)hipFree(u->d_byte_ids);
  if (u->plan_done) (void)hipEventDestroy(u->plan_done);
  if (u->h_total) (void)hipHostFree(u->h_total);
  (void)hipFree(u->d_slots);
  (void)hipFree(u->d_root);
  (void)hipFree(u->d_cont_bits);
  delete u;
}

// the text and the sentences of a call
void fill_work(UniWork* W, const uint8_t* d_text, int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent) {
  W->text = d_text;
  W->n_bytes = n_bytes;
  W->n_tiles = n_bytes / 64 + 1;  // bit n_bytes exists
  W->sent_off = d_sent_off;
  W->n_sent = n_sent;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

static_assert(kUniMaxWord == LDDL_UNIGRAM_MAX_WORD && kUniMaxNest == LDDL_UNIGRAM_MAX_NEST &&
                  kUniAsciiWs == LDDL_UNIGRAM_ASCII_WS, "the header's constants are the kernels'");

extern "C" int lddl_unigram_create(int device, const uint8_t* piece_bytes, const int64_t* piece_off,
                                   const float* scores, const int32_t* types, int64_t n_pieces,
                                   int32_t unk_id, int32_t flags, lddl_unigram** out) {
  if (!out) LDDL_FAIL(-1, "null out");
  *out = nullptr;
  if (flags & ~LDDL_UNIGRAM_ASCII_WS) LDDL_FAIL(-1, "unknown flags 0x%x", flags);
  UniHostTables H;
  if (unigram_build_tables(piece_bytes, piece_off, scores, types, n_pieces, unk_id, &H)) return -1;
  LDDL_HIP(hipSetDevice(device));
  lddl_unigram* u = new lddl_unigram;
  u->device = device;
  u->n_pieces = n_pieces;
  u->n_nodes = H.n_nodes;
  u->n_slots = (int64_t)H.slots.size();
  u->cont_host = H.cont_bits;
  int st = upload(&u->d_slots, H.slots.data(), H.slots.size() * sizeof(UniSlot));
  st = st ? st : upload(&u->d_root, H.root, sizeof(H.root));
  st = st ? st : upload(&u->d_cont_bits, H.cont_bits.data(), H.cont_bits.size() * sizeof(uint32_t));
  if (st) {
    release(u);
    return st;
  }
  u->tab = UniTables{u->d_slots, u->d_root, (uint32_t)H.slots.size() - 1, H.pre_node, H.pre_id, unk_id,
                     H.unk_score, H.pre_score, flags & LDDL_UNIGRAM_ASCII_WS};
  *out = u;
  return 0;
}

extern "C" int lddl_unigram_destroy(lddl_unigram* u) {
  if (!u) return 0;
  (void)hipSetDevice(u->device);
  (void)hipDeviceSynchronize();
  u->arena.trim();
  release(u);
  return 0;
}

extern "C" int lddl_unigram_info(const lddl_unigram* u, int64_t* n_pieces, int64_t* n_nodes,
                                 int64_t* table_bytes, float* unk_score, int32_t* max_word) {
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (n_pieces) *n_pieces = u->n_pieces;
  if (n_nodes) *n_nodes = u->n_nodes;
  if (table_bytes) *table_bytes = (u->n_slots + 256) * (int64_t)sizeof(UniSlot);
  if (unk_score) *unk_score = u->tab.unk_score;
  if (max_word) *max_word = kUniMaxWord;
  return 0;
}

extern "C" int lddl_unigram_cont_bits(const lddl_unigram* u, const uint32_t** d_bits, int64_t* n_ids) {
  if (!u || !d_bits || !n_ids) LDDL_FAIL(-1, "null argument");
  *d_bits = u->d_cont_bits;
  *n_ids = u->n_pieces;
  return 0;
}

extern "C" int lddl_unigram_tokenize(lddl_unigram* u, void* stream, const uint8_t* d_text,
                                     int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                                     const int64_t* d_doc_sent_off, int64_t n_doc, int32_t max_pieces,
                                     int32_t* d_ids, int32_t* d_sent_len) {
  (void)d_doc_sent_off;  // a document starts where a sentence does
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (n_bytes < 0 || n_sent < 0 || n_doc < 0) LDDL_FAIL(-1, "negative size");
  if (max_pieces < 1) LDDL_FAIL(-1, "max_pieces %d < 1", max_pieces);
  if (n_sent == 0) return 0;
  if ((n_bytes && !d_text) || !d_sent_off || !d_ids || !d_sent_len) LDDL_FAIL(-1, "null argument");
  hipStream_t st = as_stream(stream);
  UniTables tab = u->tab;
  if (u->norm.rule) tab.ascii_ws = 0;  // the rules decide what a space is
  UniWork W{};
  fill_work(&W, d_text, n_bytes, d_sent_off, n_sent);
  W.long_cap = n_bytes / 65 + 2;
  // one block of 64-bit words: sent_bits | alive_bits | pre_bits | long counter (these are
  // cleared), start_bits, break_bits, tile_base, the scan's scratch, sent_base, long_list; then sym
  const int64_t nt = W.n_tiles + 1, scratch = scan_scratch_elems(W.n_tiles);
  const int64_t clear_words = 3 * nt + 1;
  const int64_t words = clear_words + 3 * nt + scratch + (n_sent + 1) + W.long_cap;
  ArenaScope tmp(&u->arena, st);
  uint64_t* base;
  if (tmp.take(&base, words)) return -100;
  if (tmp.take(&W.sym, n_bytes + 64)) return -100;
  W.sent_bits = base;
  W.alive_bits = base + nt;
  W.pre_bits = base + 2 * nt;
  W.long_count = reinterpret_cast<unsigned long long*>(base + 3 * nt);
  W.start_bits = base + clear_words;
  W.break_bits = W.start_bits + nt;
  W.tile_base = reinterpret_cast<int64_t*>(W.break_bits + nt);
  int64_t* scan_tmp = W.tile_base + nt;
  W.sent_base = scan_tmp + scratch;
  W.long_list = W.sent_base + n_sent + 1;
  LDDL_HIP(unigram_launch_words(tab, W, clear_words, st));
  LDDL_HIP(unigram_launch_tiles(tab, W, st));
  LDDL_HIP(unigram_launch_long(tab, W, st));
  if (u->d_byte_ids) {  // tile_base is free until the scan: the cover words
    LDDL_HIP(unigram_launch_bytes(tab, W, u->d_byte_ids, reinterpret_cast<uint64_t*>(W.tile_base), st));
  }
  LDDL_HIP(scan_exclusive(TileCount{W.alive_bits, W.pre_bits}, W.n_tiles, W.tile_base, scan_tmp, st));
  hipLaunchKernelGGL(uni_sent_base_kernel, dim3((unsigned)(n_sent / 256 + 1)), dim3(256), 0, st, W);
  hipLaunchKernelGGL(uni_compact_kernel, dim3((unsigned)((W.n_tiles + 3) / 4)), dim3(256), 0, st, W,
                     tab.pre_id, max_pieces, d_ids);
  hipLaunchKernelGGL(uni_sent_len_kernel, dim3((unsigned)((n_sent + 255) / 256)), dim3(256), 0, st, W,
                     max_pieces, d_sent_len);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_unigram_word_stats(lddl_unigram* u, void* stream, const uint8_t* d_text,
                                       int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                                       const int64_t* d_doc_sent_off, int64_t n_doc, int64_t* d_stats) {
  (void)d_doc_sent_off;
  if (!u) LDDL_FAIL(-1, "null unigram");
  if (n_bytes < 0 || n_sent < 0 || n_doc < 0) LDDL_FAIL(-1, "negative size");
  if ((n_bytes && !d_text) || !d_sent_off || !d_stats) LDDL_FAIL(-1, "null argument");
  hipStream_t st = as_stream(stream);
  UniWork W{};
  fill_work(&W, d_text, n_bytes, d_sent_off, n_sent);
  // sent_bits | three counters (cleared by the first launch) | start_bits | break_bits
  const int64_t nt = W.n_tiles + 1, clear_words = nt + 3;
  ArenaScope tmp(&u->arena, st);
  uint64_t* base;
  if (tmp.take(&base, clear_words + 2 * nt)) return -100;
  W.sent_bits = base;
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(base + nt);
  W.start_bits = base + clear_words;
  W.break_bits = W.start_bits + nt;
  UniTables tab = u->tab;
  if (u->norm.rule) tab.ascii_ws = 0;
  LDDL_HIP(unigram_launch_words(tab, W, clear_words, st));
  hipLaunchKernelGGL(uni_stats_kernel, dim3((unsigned)((W.n_tiles + 255) / 256)), dim3(256), 0, st, W,
                     counters);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipMemcpyAsync(d_stats, counters, 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return 0;
}
