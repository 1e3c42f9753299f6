// SentencePiece unigram, the long pass: one wave per listed word (over 64 bytes),
// in slices of at most kUniMaxWord bytes cut at a character start (the stated deviation; only
// the first slice carries the prefix). A slice's bytes, character lengths, best[] and
// back-pointers sit in LDS (kUniMaxWord positions). The starts are matched 64 at a time, lane =
// start, into 64 rows of the edge table, each walk running on to a miss or the slice's end;
// then lane 0 relaxes those 64 starts in rising order, so a start's score is final when its
// edges are read. Lane 0 takes the prefix walk before the first stride and reads the path back.
// A fixed-size launch: the grid strides over the list, whose length it reads on the device.
#include "device.h"
#include "unigram.h"

namespace lddl {
namespace {

constexpr int kLongGrid = 2048;
constexpr int kLongRows = 65;  // 64 starts and the prefix

// the first break after byte x0 (a word starts at x0): the word's end
__device__ inline int64_t word_end(const UniWork& W, int64_t x0) {
  const int lane = lane_id();
  const uint64_t m0 = uni_above(W.break_bits[x0 >> 6], (int)(x0 & 63));
  if (m0) return (x0 >> 6) * 64 + __builtin_ctzll(m0);
  for (int64_t w0 = (x0 >> 6) + 1;; w0 += 64) {
    const int64_t w = w0 + lane;
    const uint64_t m = w < W.n_tiles ? W.break_bits[w] : ~0ull;
    const uint64_t B = ballot(m != 0);
    if (B) {
      const int f = __builtin_ctzll(B);
      const uint32_t l32 = (uint32_t)__shfl((int)(uint32_t)m, f, 64);
      const uint32_t h32 = (uint32_t)__shfl((int)(uint32_t)(m >> 32), f, 64);
      return (w0 + f) * 64 + __builtin_ctzll((uint64_t)h32 << 32 | l32);
    }
  }
}

__global__ void __launch_bounds__(64) uni_long_kernel(UniTables T, UniWork W) {
  __shared__ uint2 edge[kUniMaxNest * kLongRows];
  __shared__ float best[kUniMaxWord];
  __shared__ uint32_t back[kUniMaxWord];
  __shared__ uint8_t byte[kUniMaxWord], clen[kUniMaxWord], cnt[kLongRows];
  const int lane = lane_id();
  unsigned long long count = *W.long_count;
  if (count > (unsigned long long)W.long_cap) count = (unsigned long long)W.long_cap;
  for (int64_t i = blockIdx.x; i < (int64_t)count; i += gridDim.x) {
    const int64_t x0 = W.long_list[i];
    int64_t end = word_end(W, x0);
    end = end < W.n_bytes ? end : W.n_bytes;
    int n = 0;
    for (int64_t a = x0; a < end; a += n) {
      n = (int)(end - a < kUniMaxWord ? end - a : kUniMaxWord);
      wave_sync();  // the slice before is read to its end
      for (int k = lane; k < n; k += 64) {
        byte[k] = W.text[a + k];
        best[k] = -INFINITY;
      }
      wave_sync();
      if (a + n < end) {  // cut at a character start: at most three bytes back
        const int full = n;
        int more = 0;  // the bytes from `full` on that the slice's last character needs
        for (int k = 1; k <= 3; ++k) {
          const uint8_t c = byte[full - k];
          if (c >= 0xC0) {
            const int len = uni_lead_len(c);
            bool whole = a + full - k + len <= end;
            for (int q = 1; q < len && whole; ++q) whole = (W.text[a + full - k + q] & 0xC0) == 0x80;
            if (whole && len > k) more = k;
            break;
          }
          if (c < 0x80) break;
        }
        n = full - more;
      }
      for (int k = lane; k < n; k += 64) clen[k] = (uint8_t)uni_char_len(byte, k, 0, n);
      const bool head = a == x0;
      float b0 = 0.0f;  // lane 0's: the score at the slice's first byte
      if (lane == 0) {
        cnt[64] = 0;
        if (head) {
          bool none = false;
          cnt[64] = (uint8_t)uni_walk(T, byte, T.pre_node, 0, n, edge, kLongRows, 64, -1, &none);
          b0 = 0.0f + T.pre_score;
          uni_relax_row(edge, kLongRows, 64, cnt[64], 0.0f, 0u, best, back);
        }
      }
      for (int s0 = 0; s0 < n; s0 += 64) {
        wave_sync();  // clen is written; lane 0 has read the rows of the stride before
        const int p = s0 + lane;
        const int cl = p < n ? clen[p] : 0;
        bool one = false;
        cnt[lane] = cl > 0 ? (uint8_t)uni_walk(T, byte, 0, p, n, edge, kLongRows, lane, cl, &one) : 0;
        const uint64_t ONE = ballot(one);
        wave_sync();
        if (lane == 0)
          for (int q = 0; q < 64 && s0 + q < n; ++q) {
            const int pp = s0 + q, c = clen[pp];
            if (!c) continue;
            const float bs = pp == 0 ? b0 : best[pp - 1];
            if (bs == -INFINITY) continue;
            uni_relax_row(edge, kLongRows, q, cnt[q], bs, (uint32_t)pp + 1, best, back);
            if (!((ONE >> q) & 1))
              uni_relax(best, back, pp + c - 1, bs + T.unk_score, (uint32_t)T.unk_id | (uint32_t)(pp + 1) << 20);
          }
      }
      wave_sync();
      if (lane == 0) {
        bool last_unk = false;
        int64_t last_x = 0;
        for (int j = n - 1, it = 0; j >= 0 && it < kUniMaxWord; ++it) {
          const uint32_t bk = back[j];
          const int32_t id = (int32_t)(bk & 0xFFFFFu);
          const int code = (int)(bk >> 20);
          const int p = code ? code - 1 : 0;
          if (p > j || best[j] == -INFINITY) break;  // never: every character is reached
          const int64_t x = a + p;
          W.sym[x] = id;
          if (id == T.unk_id && last_unk) {
            // the run goes on to the left: its bit moves with it
            atomicAnd(reinterpret_cast<unsigned long long*>(W.alive_bits + (last_x >> 6)), ~(1ull << (last_x & 63)));
          }
          atomicOr(reinterpret_cast<unsigned long long*>(W.alive_bits + (x >> 6)), 1ull << (x & 63));
          last_unk = id == T.unk_id;
          last_x = x;
          if (p == 0) {
            if (head && code != 0)
              atomicOr(reinterpret_cast<unsigned long long*>(W.pre_bits + (x >> 6)), 1ull << (x & 63));
            break;
          }
          j = p - 1;
        }
      }
    }
  }
}

}  // namespace

hipError_t unigram_launch_long(const UniTables& T, const UniWork& W, hipStream_t st) {
  const int64_t g = W.long_cap < kLongGrid ? W.long_cap : kLongGrid;
  hipLaunchKernelGGL(uni_long_kernel, dim3((unsigned)(g > 0 ? g : 1)), dim3(64), 0, st, T, W);
  return hipGetLastError();
}

}  // namespace lddl
