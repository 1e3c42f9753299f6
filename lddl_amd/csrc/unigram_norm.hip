// SentencePiece unigram, the normaliser: lddl_unigram_normalize_plan / _write.
//
// Lane = byte, one wave per 64-byte tile. Every byte has a candidate, what the sequential scan
// would do if it stood there: the longest key that matches inside the sentence (consumed bytes,
// rule), else a well-formed character (its length, copy), else one byte for U+FFFD. The live
// bytes are the chain i -> i + consumed(i) from the sentence's first byte. A chain leaves its
// tile through the tile's `exit`, the bytes of the next tile that its last step takes, and
// enters the next one at that offset, the tile's `entry`.
//   info    per tile, no neighbour needed. One ballot finds the tiles where no byte starts a key
//           (by the 256-bit mask of one-byte keys and the 64 Kibit mask of two-byte key heads)
//           and every byte sits in a well-formed character ("cleanish"): their exit is the tail
//           of the last character and no trie is walked. A dirty tile walks the trie from every
//           byte, resolves the chain of every lane at once by pointer doubling over the wave
//           (six rounds of three lane permutes: the last lane of each chain and the set of its
//           lanes) and records the exit and up to which entry it is the same.
//   entry   lane = tile: entry(t) = exit(t - 1) wherever that exit holds for every entry a key
//           can cause. The other tiles form runs, met only where chains of different entries
//           never merge (keys `ab` and `ba` on `ababab...`); the wave walks each run in order and
//           recomputes a tile's chain from its true entry.
//   count   a cleanish tile entered at its head counts its bytes from info alone; a dirty one
//           repeats match and chain and sums the live lanes' output lengths. A sentence start is
//           live, so its lane knows the sentence's offset inside the tile's output.
//   write   after the scan of the counts, a wave per four tiles: clean tiles in a row are one
//           stretch of the text, copied a dword a lane with the stores aligned; a dirty tile
//           stages its output in LDS, kStage bytes a round, each live lane at the wave prefix sum
//           of the lengths, a replacement of more than kCoop bytes copied from the blob by the
//           whole wave, and the wave stores the stage coalesced.
// Every lane reaches every ballot, permute and wave_sync; walks and copies are predicated.
#include "device.h"
#include "scan.h"
#include "unigram_norm.h"

namespace lddl {
namespace {

constexpr int kWaves = 4;
constexpr int kStage = 256;

struct NormLds {
  uint8_t b[128];  // the tile and the 64 bytes behind it (0 past the text)
  uint8_t stage[kStage];
};

__global__ void __launch_bounds__(256) norm_clear_kernel(uint64_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ void __launch_bounds__(256) norm_mark_kernel(NormWork W) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= W.n_sent) return;
  const int64_t x = W.sent_off[s];
  if (x >= 0 && x < W.n_bytes)
    atomicOr(reinterpret_cast<unsigned long long*>(W.sent_bits + (x >> 6)), 1ull << (x & 63));
}

__device__ inline void norm_load(const NormWork& W, int64_t t, NormLds& L) {
  const int lane = lane_id();
  const int64_t x = t * 64 + lane;
  wave_sync();  // the tile before is read to its end
  L.b[lane] = x < W.n_bytes ? W.text[x] : 0;
  L.b[64 + lane] = x + 64 < W.n_bytes ? W.text[x + 64] : 0;
  wave_sync();
}

// the bytes from the lane's own to the end of its sentence, 64 at most; 0 past the text
__device__ inline int norm_limit(const NormWork& W, int64_t t) {
  const int lane = lane_id();
  const int64_t rem = W.n_bytes - (t * 64 + lane);
  if (rem <= 0) return 0;
  const uint64_t ahead = ((W.sent_bits[t] >> lane) >> 1) | (W.sent_bits[t + 1] << (63 - lane));
  const int d = ahead ? __builtin_ctzll(ahead) + 1 : 64;
  return rem < d ? (int)rem : d;
}

// the length of the well-formed UTF-8 character at b[p] within `limit` bytes, or 0
__device__ inline int norm_utf8_len(const uint8_t* b, int p, int limit) {
  const uint32_t c = b[p];
  if (c < 0x80) return 1;
  const int n = uni_lead_len(c);
  if (n == 1 || n > limit) return 0;
  const uint32_t c1 = b[p + 1];
  if ((c1 & 0xC0) != 0x80) return 0;
  if ((c == 0xE0 && c1 < 0xA0) || (c == 0xED && c1 > 0x9F) || (c == 0xF0 && c1 < 0x90) || (c == 0xF4 && c1 > 0x8F))
    return 0;  // overlong, a surrogate, past U+10FFFF
  for (int k = 2; k < n; ++k)
    if ((b[p + k] & 0xC0) != 0x80) return 0;
  return n;
}

// may a key start at b[p], `limit` bytes before its sentence's end: the byte alone is a key, or
// it and the next byte open a longer one (the NFKC map composes: `a` opens keys, `ab` does not)
__device__ inline bool norm_starts_key(const NormTables& N, const uint8_t* b, int p, int limit) {
  const uint32_t c = b[p];
  if (!((N.start[c >> 6] >> (c & 63)) & 1)) return false;
  if ((N.single[c >> 6] >> (c & 63)) & 1) return true;
  if (limit < 2) return false;
  const uint32_t d = b[p + 1];
  return (N.pair[c << 2 | d >> 6] >> (d & 63)) & 1;
}

// the lane's candidate: consumed bytes and rule (kNormCopy, kNormBad); a lane past the text
// consumes 1
__device__ inline int norm_cand(const NormTables& N, const uint8_t* b, int limit, int32_t* rule) {
  const int lane = lane_id();
  *rule = kNormCopy;
  if (limit <= 0) return 1;
  if (norm_starts_key(N, b, lane, limit)) {
    const UniTables T{N.slots, N.root, N.mask, 0u, 0, 0, 0.f, 0.f, 0};
    const int hi = limit < N.max_key ? limit : N.max_key;
    uint32_t node = 0;
    int best = 0;
    UniSlot e;
    for (int k = 0; k < hi && uni_step(T, node, b[lane + k], &e); ++k) {
      node = e.child;
      if (e.id >= 0) {
        best = k + 1;
        *rule = e.id;
      }
    }
    if (best) return best;
  }
  const int u = norm_utf8_len(b, lane, limit);
  if (u) return u;
  *rule = kNormBad;
  return 1;
}

// Pointer doubling over the chain lane -> lane + cons inside the tile: *last = the chain's last
// lane of the tile, *reach = its lanes.
__device__ inline void norm_chain(int cons, int* last, uint64_t* reach) {
  const int lane = lane_id();
  int p = lane + cons < 64 ? lane + cons : lane;
  uint64_t R = 1ull << lane | 1ull << p;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)R, p, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(R >> 32), p, 64);
    R |= (uint64_t)hi << 32 | lo;
    p = __shfl(p, p, 64);
  }
  *last = p;
  *reach = R;
}

// the exit of the chain that starts at each lane
__device__ inline int norm_exits(const NormTables& N, const NormWork& W, int64_t t, NormLds& L) {
  norm_load(W, t, L);
  int32_t rule;
  const int cons = norm_cand(N, L.b, norm_limit(W, t), &rule);
  int last;
  uint64_t R;
  norm_chain(cons, &last, &R);
  return __shfl(lane_id() + cons - 64, last, 64);
}

__global__ void __launch_bounds__(64 * kWaves) norm_info_kernel(NormTables N, NormWork W) {
  __shared__ NormLds lds[kWaves];
  const int w = wave_id(), lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * kWaves + w;
  if (t >= W.n_tiles) return;  // the whole wave; no block-wide barrier below
  NormLds& L = lds[w];
  norm_load(W, t, L);
  const int limit = norm_limit(W, t);
  const bool in = limit > 0;
  const uint32_t c = L.b[lane];
  const bool cont = in && (c & 0xC0) == 0x80;
  const int u = in && !cont ? norm_utf8_len(L.b, lane, limit) : 0;
  uint32_t info = 0;
  bool clean = !ballot(in && (norm_starts_key(N, L.b, lane, limit) || (!cont && u == 0)));
  if (clean) {
    const uint64_t U2 = ballot(u >= 2), U3 = ballot(u >= 3), U4 = ballot(u == 4), C = ballot(cont);
    const int head = ~C ? __builtin_ctzll(~C) : 64;
    const uint64_t stray = C & ~(U2 << 1 | U3 << 2 | U4 << 3);
    clean = head <= 3 && !(stray >> head);
    const int e2 = (int)(U2 >> 63), e3 = (U3 >> 63) ? 2 : (int)((U3 >> 62) & 1);
    const int e4 = (U4 >> 63) ? 3 : ((U4 >> 62) & 1) ? 2 : (int)((U4 >> 61) & 1);
    const int exit = e4 > e3 ? e4 : (e3 > e2 ? e3 : e2);
    // from any entry up to 60 the chain meets a character start inside the tile
    info = kNormCleanish | (uint32_t)head << 16 | 60u << 8 | (uint32_t)exit;
  }
  if (!clean) {
    const int X = norm_exits(N, W, t, L);
    const int X0 = __shfl(X, 0, 64);
    const uint64_t same = ballot(X == X0);
    const int upto = ~same ? __builtin_ctzll(~same) - 1 : 63;
    info = (uint32_t)upto << 8 | (uint32_t)X0;
  }
  if (lane == 0) W.info[t] = info;
}

__device__ inline int info_exit(uint32_t i) { return (int)(i & 255u); }
__device__ inline int info_upto(uint32_t i) { return (int)((i >> 8) & 255u); }
__device__ inline int info_head(uint32_t i) { return (int)((i >> 16) & 3u); }

__global__ void __launch_bounds__(64) norm_entry_kernel(NormTables N, NormWork W) {
  __shared__ NormLds L;
  const int lane = lane_id();
  const int64_t t0 = (int64_t)blockIdx.x * 64, t = t0 + lane;
  // the largest entry: a key's tail, or that of a character of four bytes
  const int most = N.max_key - 1 > 3 ? N.max_key - 1 : 3;
  const bool valid = t < W.n_tiles;
  // tile 0 is entered at 0, so tile 1 is never in doubt
  const bool hard = valid && t >= 2 && info_upto(W.info[t - 1]) < most;
  const bool before = valid && t >= 3 && info_upto(W.info[t - 2]) < most;
  if (valid && !hard) W.entry[t] = (uint8_t)(t == 0 ? 0 : info_exit(W.info[t - 1]));
  for (uint64_t heads = ballot(hard && !before); heads; heads &= heads - 1) {
    int64_t tt = t0 + __builtin_ctzll(heads);
    int e = info_exit(W.info[tt - 2]);  // the entry of tile tt - 1, which is not in doubt
    do {
      const uint32_t prev = W.info[tt - 1];
      e = e <= info_upto(prev) ? info_exit(prev) : __shfl(norm_exits(N, W, tt - 1, L), e, 64);
      if (lane == 0) W.entry[tt] = (uint8_t)e;
      ++tt;
    } while (tt < W.n_tiles && info_upto(W.info[tt - 1]) < most);
  }
}

// What a tile's lanes emit, given its entry: *len bytes each (0: not live) of *rule, *cons for a
// copy; returns the wave's inclusive prefix sum of the lengths. L.b holds the tile afterwards.
__device__ inline int norm_emit(const NormTables& N, const NormWork& W, int64_t t, int entry, NormLds& L,
                                int* len, int32_t* rule) {
  const int lane = lane_id();
  norm_load(W, t, L);
  const int limit = norm_limit(W, t);
  const int cons = norm_cand(N, L.b, limit, rule);
  int last;
  uint64_t R;
  norm_chain(cons, &last, &R);
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)R, entry, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(R >> 32), entry, 64);
  const bool live = limit > 0 && lane >= entry && (((uint64_t)hi << 32 | lo) >> lane) & 1;
  *len = !live ? 0 : *rule >= 0 ? (int)N.rule[*rule].len : *rule == kNormCopy ? cons : 3;
  return wave_incl_scan(*len);
}

__device__ inline bool norm_fast(uint32_t info, int entry) { return (info & kNormCleanish) && entry == info_head(info); }

__global__ void __launch_bounds__(64 * kWaves) norm_count_kernel(NormTables N, NormWork W, int64_t* out_sent_off) {
  __shared__ NormLds lds[kWaves];
  const int w = wave_id(), lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * kWaves + w;
  if (t >= W.n_tiles) return;
  const uint32_t info = W.info[t];
  const int entry = W.entry[t];
  int before, count;  // the output bytes of the lanes below this one, and of the tile
  if (norm_fast(info, entry)) {
    const int64_t rem = W.n_bytes - t * 64;
    before = lane - entry;
    count = (int)(rem < 64 ? rem : 64) - entry + info_exit(info);
  } else {
    int len;
    int32_t rule;
    const int incl = norm_emit(N, W, t, entry, lds[w], &len, &rule);
    before = incl - len;
    count = __shfl(incl, 63, 64);
  }
  if (lane == 0) W.count[t] = count;
  if ((W.sent_bits[t] >> lane) & 1) {  // every sentence that starts at this byte
    const int64_t x = t * 64 + lane;
    int64_t lo = 0, hi = W.n_sent;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (W.sent_off[mid] < x) lo = mid + 1;
      else hi = mid;
    }
    for (; lo < W.n_sent && W.sent_off[lo] == x; ++lo) out_sent_off[lo] = before;
  }
}

struct NormTileCount {
  const int32_t* count;
  __device__ int64_t operator()(int64_t t) const { return count[t]; }
};

__global__ void __launch_bounds__(256) norm_sent_off_kernel(NormWork W, int64_t* out_sent_off) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > W.n_sent) return;
  const int64_t x = s < W.n_sent ? W.sent_off[s] : W.n_bytes;
  out_sent_off[s] = x >= W.n_bytes ? W.tile_base[W.n_tiles] : x < 0 ? 0 : out_sent_off[s] + W.tile_base[x >> 6];
}

// n <= 259 bytes text[src, src + n) -> out[dst, dst + n), by the wave: the dwords of `out` that
// lie inside are stored whole, one a lane, each from the two aligned source words around it
// (v_alignbyte); the up to three bytes before and behind them go bytewise. A source word that
// would reach outside text[0, n_bytes) is read bytewise instead. No store at or past out_cap.
__device__ inline void norm_wave_copy(uint8_t* out, int64_t dst, int64_t out_cap, const uint8_t* text,
                                      int64_t n_bytes, int64_t src, int n) {
  const int lane = lane_id();
  const uint8_t* s = text + src;
  if (dst + n > out_cap) {
    for (int j = lane; j < n; j += 64)
      if (dst + j < out_cap) out[dst + j] = s[j];
    return;
  }
  uint8_t* d = out + dst;
  const int skew = (int)(-reinterpret_cast<uintptr_t>(d) & 3);
  const int head = skew < n ? skew : n, nd = (n - head) >> 2, tail = n - head - 4 * nd;
  if (lane < nd) {
    const uint8_t* sp = s + head + 4 * lane;
    const int sh = (int)(reinterpret_cast<uintptr_t>(sp) & 3);
    const uint8_t* lo = sp - sh;
    uint32_t v;
    if (reinterpret_cast<uintptr_t>(lo) >= reinterpret_cast<uintptr_t>(text) && lo + (sh ? 8 : 4) <= text + n_bytes) {
      const uint32_t a = *reinterpret_cast<const uint32_t*>(lo);
      const uint32_t b = sh ? *reinterpret_cast<const uint32_t*>(lo + 4) : 0u;
      v = __builtin_amdgcn_alignbyte(b, a, (uint32_t)sh);
    } else {
      v = (uint32_t)sp[0] | (uint32_t)sp[1] << 8 | (uint32_t)sp[2] << 16 | (uint32_t)sp[3] << 24;
    }
    *reinterpret_cast<uint32_t*>(d + head + 4 * lane) = v;
  }
  if (lane < head) d[lane] = s[lane];
  if (lane < tail) d[head + 4 * nd + lane] = s[head + 4 * nd + lane];
}

constexpr int kCoop = 8;  // a replacement longer than this is copied by the whole wave

// a dirty tile: the output staged in LDS, kStage bytes a round
__device__ inline void norm_write_dirty(const NormTables& N, const NormWork& W, int64_t t, int entry, int64_t dst,
                                        NormLds& L, uint8_t* out, int64_t out_cap) {
  const int lane = lane_id();
  int len;
  int32_t rule;
  const int incl = norm_emit(N, W, t, entry, L, &len, &rule);
  const int at = incl - len, total = __shfl(incl, 63, 64);
  const int roff = rule >= 0 ? (int)N.rule[rule].off : 0;
  const bool coop = rule >= 0 && len > kCoop;
  const uint64_t COOP = ballot(coop);
  const uint8_t* from = rule >= 0 ? N.repl + roff : L.b + lane;
  for (int r0 = 0; r0 < total; r0 += kStage) {
    wave_sync();  // the round before is stored
    if (!coop) {
      const int lo = at > r0 ? at : r0, hi = at + len < r0 + kStage ? at + len : r0 + kStage;
      for (int k = lo; k < hi; ++k) {
        const int q = k - at;
        L.stage[k - r0] = rule == kNormBad ? (q == 0 ? 0xEF : q == 1 ? 0xBF : 0xBD) : from[q];
      }
    }
    for (uint64_t m = COOP; m; m &= m - 1) {  // lane = byte of the replacement
      const int l = __builtin_ctzll(m);
      const int a = __shfl(at, l, 64), n = __shfl(len, l, 64), off = __shfl(roff, l, 64);
      const int lo = a > r0 ? a : r0, hi = a + n < r0 + kStage ? a + n : r0 + kStage;
      for (int k = lo + lane; k < hi; k += 64) L.stage[k - r0] = N.repl[off + k - a];
    }
    wave_sync();
    const int n = total - r0 < kStage ? total - r0 : kStage;
    for (int j = lane; j < n; j += 64)
      if (dst + r0 + j < out_cap) out[dst + r0 + j] = L.stage[j];
  }
}

constexpr int kGroup = 4;  // tiles a wave of the write takes: 64 dwords if all are clean

__global__ void __launch_bounds__(64 * kWaves) norm_write_kernel(NormTables N, NormWork W, uint8_t* out,
                                                                 int64_t out_cap) {
  __shared__ NormLds lds[kWaves];
  const int w = wave_id(), lane = lane_id();
  const int64_t t0 = ((int64_t)blockIdx.x * kWaves + w) * kGroup;
  if (t0 >= W.n_tiles) return;
  const int nt = W.n_tiles - t0 < kGroup ? (int)(W.n_tiles - t0) : kGroup;
  uint32_t info = 0;
  int entry = 0;
  if (lane < nt) {
    info = W.info[t0 + lane];
    entry = W.entry[t0 + lane];
  }
  const uint64_t fast = ballot(lane < nt && norm_fast(info, entry));
  if (fast == (1ull << nt) - 1) {
    // clean tiles in a row are one stretch of the text: each ends where the next is entered
    const int64_t dst = W.tile_base[t0];
    norm_wave_copy(out, dst, out_cap, W.text, W.n_bytes, t0 * 64 + __shfl(entry, 0, 64),
                   (int)(W.tile_base[t0 + nt] - dst));
    return;
  }
  for (int k = 0; k < nt; ++k) {
    const int64_t t = t0 + k, dst = W.tile_base[t];
    const int e = __shfl(entry, k, 64);
    if ((fast >> k) & 1) norm_wave_copy(out, dst, out_cap, W.text, W.n_bytes, t * 64 + e, W.count[t]);
    else norm_write_dirty(N, W, t, e, dst, lds[w], out, out_cap);
  }
}

// lddl_unigram_normalize_stats: stats[0] the tiles, stats[1] those that take the dirty path
__global__ void __launch_bounds__(256) norm_stats_kernel(NormWork W, unsigned long long* stats) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t dirty = ballot(t < W.n_tiles && !norm_fast(W.info[t < W.n_tiles ? t : 0], W.entry[t < W.n_tiles ? t : 0]));
  if (lane_id() == 0 && dirty) atomicAdd(stats + 1, (unsigned long long)__popcll(dirty));
  if (t == 0) atomicAdd(stats, (unsigned long long)W.n_tiles);
}

inline dim3 tile_grid(int64_t n_tiles) { return dim3((unsigned)((n_tiles + kWaves - 1) / kWaves)); }

}  // namespace

hipError_t unigram_norm_launch_plan(const NormTables& N, const NormWork& W, int64_t* scan_tmp,
                                    int64_t* out_sent_off, hipStream_t st) {
  const int64_t words = W.n_tiles + 2;
  hipLaunchKernelGGL(norm_clear_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, W.sent_bits, words);
  if (W.n_sent > 0)
    hipLaunchKernelGGL(norm_mark_kernel, dim3((unsigned)((W.n_sent + 255) / 256)), dim3(256), 0, st, W);
  if (W.n_tiles > 0) {
    hipLaunchKernelGGL(norm_info_kernel, tile_grid(W.n_tiles), dim3(64 * kWaves), 0, st, N, W);
    hipLaunchKernelGGL(norm_entry_kernel, dim3((unsigned)((W.n_tiles + 63) / 64)), dim3(64), 0, st, N, W);
    hipLaunchKernelGGL(norm_count_kernel, tile_grid(W.n_tiles), dim3(64 * kWaves), 0, st, N, W, out_sent_off);
  }
  hipError_t e = scan_exclusive(NormTileCount{W.count}, W.n_tiles, W.tile_base, scan_tmp, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(norm_sent_off_kernel, dim3((unsigned)(W.n_sent / 256 + 1)), dim3(256), 0, st, W, out_sent_off);
  return hipGetLastError();
}

hipError_t unigram_norm_launch_write(const NormTables& N, const NormWork& W, uint8_t* out_text,
                                     int64_t out_cap, hipStream_t st) {
  if (W.n_tiles > 0)
    hipLaunchKernelGGL(norm_write_kernel, tile_grid((W.n_tiles + kGroup - 1) / kGroup), dim3(64 * kWaves), 0, st, N,
                       W, out_text, out_cap);
  return hipGetLastError();
}

hipError_t unigram_norm_launch_stats(const NormWork& W, int64_t* d_stats, hipStream_t st) {
  hipLaunchKernelGGL(norm_clear_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<uint64_t*>(d_stats), (int64_t)2);
  if (W.n_tiles > 0)
    hipLaunchKernelGGL(norm_stats_kernel, dim3((unsigned)((W.n_tiles + 255) / 256)), dim3(256), 0, st, W,
                       reinterpret_cast<unsigned long long*>(d_stats));
  return hipGetLastError();
}

}  // namespace lddl
