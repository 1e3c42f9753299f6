// SentencePiece unigram, the words and the tile pass.
//
// Words: lane = byte. A byte breaks (a space, a sentence start, past the text) or not; a word
// starts at a non-space byte behind a space, at a sentence start or at byte 0 and ends before
// the next break. One ballot each writes the start mask and the break mask of a 64-byte tile.
//
// Tile pass: one wave per tile, which owns the words that start in it. A window is 64 bytes,
// lane = byte; the first window is the tile and holds the owned words that end in it, the
// second, if there is one, starts at the first byte of the one owned word that crosses the
// tile's end and holds that word alone (a word over 64 bytes goes to the long list of
// unigram_viterbi.hip). In a window:
//   match    every lane at a character start walks the trie from the root along its own bytes
//            to a miss or its word's end; a free lane right before a word's first byte walks
//            from the node of the prefix E2 96 81 along that word; the words without such a
//            lane (at the window's first lane, behind a sentence start) take that walk in a
//            second round, which a ballot enters. A walk appends (end, id, score) to its row of
//            the wave's LDS edge table, 64 root rows and 64 prefix rows of kUniMaxNest edges,
//            and keeps the count in a register; "a piece of exactly one character matched
//            here" is one bit per lane.
//   Viterbi  the lane of a word's first byte sweeps its word: best[] and the back-pointers sit
//            in LDS, one slot per byte (a path that ends behind byte j), so the words of a
//            window never share a slot; the score behind the prefix alone is a register. Single
//            float32 adds, strictly greater replaces, starts in rising order.
//   path     read back from the word's last byte: sym[x] = id at the piece's first byte, one
//            bit of alive_bits, unknown runs keep their first bit only, and a bit of pre_bits
//            where the prefix piece stands alone before the piece at the word's first byte.
// Every lane reaches every ballot and wave_sync; the walks and sweeps are predicated.
#include "device.h"
#include "unigram.h"

namespace lddl {
namespace {

constexpr int kTileWaves = 2;  // 17 KiB of LDS a wave
constexpr int kRows = 128;     // root rows 0 .. 63, prefix rows 64 .. 127

__global__ void __launch_bounds__(256) uni_clear_kernel(uint64_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ void __launch_bounds__(256) uni_mark_sents_kernel(UniWork W) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= W.n_sent) return;
  const int64_t x = W.sent_off[s];
  if (x >= 0 && x < W.n_bytes)
    atomicOr(reinterpret_cast<unsigned long long*>(W.sent_bits + (x >> 6)), 1ull << (x & 63));
}

__global__ void __launch_bounds__(256) uni_words_kernel(UniTables T, UniWork W) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool inside = x < W.n_bytes;
  const bool sp = !inside || uni_space(T, W.text[x]);
  const bool ss = inside && ((W.sent_bits[x >> 6] >> (x & 63)) & 1);
  const bool after = x == 0 || ss || (inside && uni_space(T, W.text[x - 1]));
  const uint64_t S = ballot(!sp && after), B = ballot(sp || ss);
  const int64_t tile = x >> 6;
  if (lane_id() == 0 && tile < W.n_tiles) {
    W.start_bits[tile] = S;
    W.break_bits[tile] = B;
  }
}

struct WaveLds {
  uint2 edge[kUniMaxNest * kRows];
  float best[64];
  uint32_t back[64];
  uint8_t cnt[kRows];
  uint8_t byte[64], clen[64];
};

__device__ inline uint64_t wave_or(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, d, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, d, 64);
  }
  return (uint64_t)hi << 32 | lo;
}

// One window, lane = byte `first + lane`: the lanes with `in` belong to whole words [ws, we)
// (window lanes, we <= 64).
__device__ inline void uni_window(const UniTables& T, const UniWork& W, int64_t first, bool in,
                                  int ws, int we, WaveLds& L) {
  const int lane = lane_id();
  wave_sync();  // the window before is read to its end
  L.byte[lane] = first + lane < W.n_bytes ? W.text[first + lane] : 0x20;
  L.best[lane] = -INFINITY;
  wave_sync();
  const int cl = in ? uni_char_len(L.byte, lane, ws, we) : 0;
  L.clen[lane] = (uint8_t)cl;
  // ---- match ----
  const bool word_first = in && lane == ws;
  const uint64_t F = ballot(word_first);
  const bool helper = !in && lane < 63 && ((F >> (lane + 1)) & 1);
  const int we_next = __shfl(we, (lane + 1) & 63, 64);
  bool one = false, none = false;
  if (in && cl > 0) L.cnt[lane] = (uint8_t)uni_walk(T, L.byte, 0, lane, we, L.edge, kRows, lane, cl, &one);
  else L.cnt[lane] = 0;
  if (helper)
    L.cnt[64 + lane + 1] = (uint8_t)uni_walk(T, L.byte, T.pre_node, lane + 1, we_next, L.edge, kRows,
                                             64 + lane + 1, -1, &none);
  const uint64_t H = ballot(helper) << 1;
  const bool own_prefix = word_first && !((H >> lane) & 1);
  if (ballot(own_prefix) && own_prefix)
    L.cnt[64 + lane] = (uint8_t)uni_walk(T, L.byte, T.pre_node, lane, we, L.edge, kRows, 64 + lane, -1, &none);
  const uint64_t ONE = ballot(one);
  wave_sync();
  // ---- Viterbi and the path, lane = word ----
  uint64_t alive = 0;
  bool pre = false;
  if (word_first) {
    const float b0 = 0.0f + T.pre_score;  // behind the prefix piece alone
    uni_relax_row(L.edge, kRows, 64 + ws, L.cnt[64 + ws], 0.0f, 0u, L.best, L.back);
    for (int p = ws; p < we; ++p) {
      const int c = L.clen[p];
      if (!c) continue;
      const float bs = p == ws ? b0 : L.best[p - 1];
      if (bs == -INFINITY) continue;
      uni_relax_row(L.edge, kRows, p, L.cnt[p], bs, (uint32_t)p + 1, L.best, L.back);
      if (!((ONE >> p) & 1))
        uni_relax(L.best, L.back, p + c - 1, bs + T.unk_score, (uint32_t)T.unk_id | (uint32_t)(p + 1) << 20);
    }
    bool last_unk = false;
    int last_p = 0;
    for (int j = we - 1, it = 0; j >= ws && it < 64; ++it) {
      const uint32_t bk = L.back[j];
      const int32_t id = (int32_t)(bk & 0xFFFFFu);
      const int code = (int)(bk >> 20);
      const int p = code ? code - 1 : ws;
      if (p < ws || p > j || L.best[j] == -INFINITY) break;  // never: every character is reached
      W.sym[first + p] = id;
      alive |= 1ull << p;
      if (id == T.unk_id && last_unk) alive &= ~(1ull << last_p);
      last_unk = id == T.unk_id;
      last_p = p;
      if (p == ws) {
        pre = code != 0;
        break;
      }
      j = p - 1;
    }
  }
  const uint64_t A = wave_or(alive), P = ballot(pre);
  if (lane == 0) {
    uni_or_bits(W.alive_bits, first, A);
    uni_or_bits(W.pre_bits, first, P);
  }
}

__global__ void __launch_bounds__(64 * kTileWaves) uni_tile_kernel(UniTables T, UniWork W) {
  __shared__ WaveLds lds[kTileWaves];
  const int w = wave_id(), lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * kTileWaves + w;
  if (t >= W.n_tiles) return;  // the whole wave; no block-wide barrier below
  const int64_t base = t * 64;
  const uint64_t S = W.start_bits[t], B = W.break_bits[t];
  if (!S) return;
  const uint64_t Bn = t + 1 < W.n_tiles ? W.break_bits[t + 1] : ~0ull;
  const uint64_t lo = uni_upto(S, lane);
  const int ws = lo ? 63 - __builtin_clzll(lo) : -1;
  const uint64_t hi = ws >= 0 ? uni_above(B, ws) : 0;
  const int we = hi ? __builtin_ctzll(hi) : ((Bn & 1) ? 64 : 65);  // 65: past the tile
  const bool in = ws >= 0 && lane < we && we <= 64;
  uni_window(T, W, base, in, ws, we, lds[w]);
  // the straddler: the tile's last start, if its word does not end with the tile
  const int js = 63 - __builtin_clzll(S);
  if (uni_above(B, js) || (Bn & 1)) return;
  const int len = Bn ? 64 - js + __builtin_ctzll(Bn) : 129;
  if (len <= 64) {
    uni_window(T, W, base + js, lane < len, 0, len, lds[w]);
  } else if (lane == 0) {
    const unsigned long long k = atomicAdd(W.long_count, 1ull);
    if ((int64_t)k < W.long_cap) W.long_list[k] = base + js;
  }
}

}  // namespace

hipError_t unigram_launch_words(const UniTables& T, const UniWork& W, int64_t clear_words, hipStream_t st) {
  hipLaunchKernelGGL(uni_clear_kernel, dim3((unsigned)((clear_words + 255) / 256)), dim3(256), 0, st,
                     W.sent_bits, clear_words);
  if (W.n_sent > 0)
    hipLaunchKernelGGL(uni_mark_sents_kernel, dim3((unsigned)((W.n_sent + 255) / 256)), dim3(256), 0, st, W);
  hipLaunchKernelGGL(uni_words_kernel, dim3((unsigned)((W.n_tiles + 3) / 4)), dim3(256), 0, st, T, W);
  return hipGetLastError();
}

hipError_t unigram_launch_tiles(const UniTables& T, const UniWork& W, hipStream_t st) {
  hipLaunchKernelGGL(uni_tile_kernel, dim3((unsigned)((W.n_tiles + kTileWaves - 1) / kTileWaves)),
                     dim3(64 * kTileWaves), 0, st, T, W);
  return hipGetLastError();
}

}  // namespace lddl
