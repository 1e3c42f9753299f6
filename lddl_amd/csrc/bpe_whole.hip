// Byte-level BPE, whole words (`ignore_merges` of a Hugging Face tokenizer.json, as
// Llama 3 sets it): a pre-token of at most kBpeMaxWord bytes whose bytes are a vocabulary entry
// is that entry, whatever the merges made of it. A pass of its own between bpe_merge.hip and the
// compaction: a hit leaves the token at sym[first byte] and clears the word's other alive bits.
//
// Tile pass, the shape of the merge's: one wave per 64-byte tile, lane = byte, the pre-tokens
// that start in the tile; the one that runs past its end gets a window of its own from its first
// byte. The hash of a word is a polynomial in its bytes (bpe.h), so one segmented scan over the
// wave (six steps of two 64-bit shuffles, a lane stops combining at its word's first lane) leaves
// every word's hash in its last lane. All lanes of a word probe the same slots in step; on equal
// hash and length each lane compares its byte with the token's, and one ballot says whether the
// word is that token.
// Long pass: the merge's list of the pre-tokens over 64 bytes; one wave per word, the hash and
// the compare in strides of 64 (Llama 3 has runs of spaces of more than 64 bytes as tokens).
#include "bpe.h"
#include "device.h"

namespace lddl {
namespace {

constexpr int kWholeWaves = 4;
constexpr int kWholeLongGrid = 2048;

__device__ inline uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return (uint64_t)hi << 32 | lo;
}

// the hash of the bytes of lanes ws .. lane (ws <= lane, the same for all lanes of a word);
// *pw = kBpeWordP ^ (lane - ws + 1). Every lane takes part.
__device__ inline uint64_t seg_hash(uint32_t byte, int ws, uint64_t* pw) {
  const int lane = lane_id();
  uint64_t h = byte + 1, a = kBpeWordP;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t hs = shfl_u64(h, (lane - d) & 63), as = shfl_u64(a, (lane - d) & 63);
    if (lane - d >= ws) {
      h = hs * a + h;
      a = as * a;
    }
  }
  *pw = a;
  return h;
}

__device__ inline void and_not_bits(uint64_t* bits, int64_t first, uint64_t m) {
  if (!m) return;
  const int sh = (int)(first & 63);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(bits + (first >> 6));
  if (m << sh) atomicAnd(w, ~(m << sh));
  if (sh && (m >> (64 - sh))) atomicAnd(w + 1, ~(m >> (64 - sh)));
}

// One window, lane = byte `first + lane`: the lanes with `in` belong to whole words [ws, we).
__device__ inline void whole_window(const BpeWordTable& V, const BpeWork& W, int64_t first, bool in,
                                    int ws, int we) {
  const int lane = lane_id();
  in = in && we - ws >= 2;  // a single byte is its base token already
  const uint32_t byte = in ? W.text[first + lane] : 0u;
  const uint32_t len = in ? (uint32_t)(we - ws) : 0u;
  uint64_t pw;
  const uint64_t h = seg_hash(byte, in ? ws : lane, &pw);
  const uint64_t wh = shfl_u64(h, in ? we - 1 : lane);
  const uint64_t word = in ? bpe_upto(~0ull, we - 1) & (~0ull << ws) : 0ull;
  uint32_t slot = bpe_word_slot(wh) & V.mask;
  uint32_t id = kBpeEmpty;
  bool pend = in;
  while (ballot(pend)) {
    bool cmp = false, differs = false;
    BpeWord e{};
    if (pend) {
      e = V.slots[slot];
      if (e.id == kBpeEmpty) {
        pend = false;
      } else if (e.hash == wh && e.len == len) {
        cmp = true;
        differs = V.bytes[V.off[e.id] + (lane - ws)] != byte;
      }
    }
    const uint64_t D = ballot(cmp && differs);  // the lanes of a word decide alike
    if (cmp && !(D & word)) {
      id = e.id;
      pend = false;
    }
    slot = (slot + 1) & V.mask;
  }
  const bool hit = id != kBpeEmpty;
  if (hit && lane == ws) W.sym[first + lane] = (int32_t)id;
  const uint64_t C = ballot(hit && lane != ws);
  if (lane == 0) and_not_bits(W.alive_bits, first, C);
}

__global__ void __launch_bounds__(64 * kWholeWaves) bpe_whole_tile_kernel(BpeWordTable V, BpeWork W) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * kWholeWaves + wave_id();
  if (t >= W.n_tiles) return;
  const int64_t base = t * 64;
  const uint64_t M = W.start_bits[t];
  const uint64_t Mn = t + 1 < W.n_tiles ? W.start_bits[t + 1] : ~0ull;
  const uint64_t lo = bpe_upto(M, lane), hi = bpe_above(M, lane);
  const int ws = lo ? 63 - __builtin_clzll(lo) : -1;
  const int we = hi ? __builtin_ctzll(hi) : ((Mn & 1) ? 64 : 65);  // 65: past the tile
  const bool in = base + lane < W.n_bytes && ws >= 0 && we <= 64;
  whole_window(V, W, base, in, ws, we);
  // the straddler: the tile's last start, if its word does not end with the tile (the merge
  // pushed it on the long list if it has more than 64 bytes)
  if (!M || (Mn & 1)) return;
  const int js = 63 - __builtin_clzll(M);
  if (base + js >= W.n_bytes) return;
  const int len = Mn ? 64 - js + __builtin_ctzll(Mn) : 129;
  if (len <= 64) whole_window(V, W, base + js, lane < len, 0, len);
}

// the first pre-token start after byte x0 (x0 starts one): the word's end (as in bpe_merge.hip)
__device__ inline int64_t word_end(const BpeWork& W, int64_t x0) {
  const int lane = lane_id();
  const uint64_t m0 = bpe_above(W.start_bits[x0 >> 6], (int)(x0 & 63));
  if (m0) return (x0 >> 6) * 64 + __builtin_ctzll(m0);
  for (int64_t w0 = (x0 >> 6) + 1;; w0 += 64) {
    const int64_t w = w0 + lane;
    const uint64_t m = w < W.n_tiles ? W.start_bits[w] : ~0ull;
    const uint64_t B = ballot(m != 0);
    if (B) {
      const int f = __builtin_ctzll(B);
      return (w0 + f) * 64 + __builtin_ctzll(shfl_u64(m, f));
    }
  }
}

__global__ void __launch_bounds__(64) bpe_whole_long_kernel(BpeWordTable V, BpeWork W) {
  const int lane = lane_id();
  unsigned long long count = *W.long_count;
  if (count > (unsigned long long)W.long_cap) count = (unsigned long long)W.long_cap;
  for (int64_t i = blockIdx.x; i < (int64_t)count; i += gridDim.x) {
    const int64_t x0 = W.long_list[i];
    int64_t end = word_end(W, x0);
    end = end < W.n_bytes ? end : W.n_bytes;
    const int64_t n = end - x0;
    if (n < 2 || n > kBpeMaxWord) continue;  // a longer one is merged in slices, as stated
    uint64_t wh = 0;
    for (int64_t a = 0; a < n; a += 64) {
      const int cnt = (int)(n - a < 64 ? n - a : 64);
      uint64_t pw;
      const uint64_t h = seg_hash(lane < cnt ? W.text[x0 + a + lane] : 0u, 0, &pw);
      wh = wh * shfl_u64(pw, cnt - 1) + shfl_u64(h, cnt - 1);
    }
    uint32_t id = kBpeEmpty;
    for (uint32_t slot = bpe_word_slot(wh) & V.mask;; slot = (slot + 1) & V.mask) {
      const BpeWord e = V.slots[slot];  // the same slot in every lane
      if (e.id == kBpeEmpty) break;
      if (e.hash != wh || e.len != (uint32_t)n) continue;
      const uint8_t* tok = V.bytes + V.off[e.id];
      bool differs = false;
      for (int64_t k = lane; k < n; k += 64) differs |= tok[k] != W.text[x0 + k];
      if (!ballot(differs)) {
        id = e.id;
        break;
      }
    }
    if (id == kBpeEmpty) continue;
    if (lane == 0) W.sym[x0] = (int32_t)id;
    // clear the alive bits of bytes x0 + 1 .. end - 1, lane = 64-bit word
    const int64_t w = ((x0 + 1) >> 6) + lane;
    if (w <= ((end - 1) >> 6)) {
      const int64_t lo = x0 + 1 > w * 64 ? x0 + 1 - w * 64 : 0;
      const int64_t hi = end < (w + 1) * 64 ? end - w * 64 : 64;  // 1 .. 64
      const uint64_t m = (hi == 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1);
      atomicAnd(reinterpret_cast<unsigned long long*>(W.alive_bits + w), ~m);
    }
  }
}

}  // namespace

hipError_t bpe_launch_whole(const BpeWordTable& V, const BpeWork& W, hipStream_t st) {
  hipLaunchKernelGGL(bpe_whole_tile_kernel, dim3((unsigned)((W.n_tiles + kWholeWaves - 1) / kWholeWaves)),
                     dim3(64 * kWholeWaves), 0, st, V, W);
  const int64_t g = W.long_cap < kWholeLongGrid ? W.long_cap : kWholeLongGrid;
  hipLaunchKernelGGL(bpe_whole_long_kernel, dim3((unsigned)(g > 0 ? g : 1)), dim3(64), 0, st, V, W);
  return hipGetLastError();
}

}  // namespace lddl
