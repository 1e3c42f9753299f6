// Byte-level BPE, the merges: every pre-token starts as its bytes and, round by
// round, the adjacent pair of lowest rank has ALL its occurrences merged, left to right without
// overlap (GPT-2's bpe(); one leftmost pair per round is not the same for every merge list: a
// token that two lines produce can bring in a pair of lower rank than the round's).
//
// Tile pass: one wave per 64-byte tile, lane = byte = one symbol (id, alive) in registers. The
// wave owns the pre-tokens that start in its tile; those that also end in it are merged
// together, every word at its own minimum:
//   neighbours  the next alive lane from the alive ballot (two bit operations), inside the word
//               iff it lies below the word's end, which the start mask gives once; its id by
//               ds_bpermute;
//   ranks       a probe of the (left, right) -> (rank, merged) table in global memory (L2); the
//               rank stays in a register and only a lane whose own id or right neighbour
//               changed probes again;
//   word min    ds_min_u32 into one LDS slot per word (its first lane's);
//   occurrences the lanes at the word's minimum hold the same pair; two of them overlap only in
//               a run of one repeated symbol, where the 1st, 3rd, ... of the run merge: a lane
//               counts the candidates between its run's first lane and itself by popcount;
//   the rounds  end when a ballot shows no ranked pair in the tile.
// The one owned word that runs past the tile's end goes through the same loop once more, lane =
// symbol from its first byte, if it is at most 64 bytes long; a longer one is pushed on a list.
// Long pass: one wave per listed word, in slices of kBpeMaxWord bytes (the stated deviation): the
// symbols sit in LDS, every round probes all pairs in strides of 64, takes the wave minimum,
// and compacts by ballot and popcount, the run parity carried from one stride to the next.
// A piece is left as sym[first byte] and one bit of alive_bits (atomicOr: a tile's word of bits
// also takes the tail of the straddler before it). Every lane reaches every ballot and
// cross-lane step; the tails are predicated.
#include "bpe.h"
#include "device.h"

namespace lddl {
namespace {

constexpr int kMergeWaves = 4;
constexpr int kLongGrid = 2048;

__device__ inline void probe(const BpeTables& T, uint32_t l, uint32_t r, uint32_t* rank, uint32_t* merged) {
  uint32_t h = bpe_pair_hash(l, r) & T.pair_mask;
  for (;;) {
    const uint4 e = *reinterpret_cast<const uint4*>(T.pairs + h);
    if (e.x == kBpeEmpty) {
      *rank = kBpeNoRank;
      return;
    }
    if (e.x == l && e.y == r) {
      *rank = e.z;
      *merged = e.w;
      return;
    }
    h = (h + 1) & T.pair_mask;
  }
}

__device__ inline void or_bits(uint64_t* bits, int64_t first, uint64_t m) {
  if (!m) return;
  const int sh = (int)(first & 63);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(bits + (first >> 6));
  if (m << sh) atomicOr(w, m << sh);
  if (sh && (m >> (64 - sh))) atomicOr(w + 1, m >> (64 - sh));
}

// One window of up to 64 symbols, lane = byte `first + lane`: the lanes with `in` belong to
// whole words [ws, we) (window lanes). slot: 64 words of LDS of this wave.
__device__ inline void merge_window(const BpeTables& T, const BpeWork& W, int64_t first, bool in,
                                    int ws, int we, uint32_t* slot) {
  const int lane = lane_id();
  uint32_t id = in ? (uint32_t)T.byte_id[W.text[first + lane]] : 0u;
  bool alive = in, need = in;
  uint32_t rank = kBpeNoRank, merged = 0;
  const int my_slot = in ? ws : lane;
  for (;;) {
    const uint64_t A = ballot(alive);
    const uint64_t hi = bpe_above(A, lane);
    const int r = hi ? __builtin_ctzll(hi) : 64;
    const bool has_r = alive && r < we;
    const uint32_t rid = (uint32_t)__shfl((int)id, r & 63, 64);
    if (need) {
      rank = kBpeNoRank;
      if (has_r) probe(T, id, rid, &rank, &merged);
    }
    slot[lane] = kBpeNoRank;
    wave_sync();
    if (alive && rank != kBpeNoRank) atomicMin(&slot[my_slot], rank);
    wave_sync();
    const uint32_t wmin = slot[my_slot];
    wave_sync();
    const bool cand = alive && rank != kBpeNoRank && rank == wmin;
    const uint64_t C = ballot(cand);
    if (!C) break;
    const uint64_t lo = A & ((1ull << lane) - 1);
    const int l = lo ? 63 - __builtin_clzll(lo) : -1;
    const bool lcand = alive && l >= 0 && ((C >> l) & 1);  // then l's pair is (l, this lane)
    const uint64_t RS = ballot(cand && !lcand);
    const uint64_t rs_lo = bpe_upto(RS, lane);
    const int s = rs_lo ? 63 - __builtin_clzll(rs_lo) : 0;
    const int before = __popcll(C & ((1ull << lane) - 1) & ~((1ull << s) - 1));
    const bool sel = cand && !(before & 1);
    const uint64_t SEL = ballot(sel);
    const bool dies = alive && l >= 0 && ((SEL >> l) & 1);
    if (sel) id = merged;
    if (dies) alive = false;
    const uint64_t hi2 = bpe_above(A & ~ballot(dies), lane);
    const int r2 = hi2 ? __builtin_ctzll(hi2) : 64;
    need = alive && (sel || (r2 < 64 && ((SEL >> r2) & 1)));
  }
  if (alive) W.sym[first + lane] = (int32_t)id;
  const uint64_t A = ballot(alive);
  if (lane == 0) or_bits(W.alive_bits, first, A);
}

__global__ void __launch_bounds__(64 * kMergeWaves) bpe_merge_tile_kernel(BpeTables T, BpeWork W) {
  __shared__ uint32_t slots[kMergeWaves][64];
  const int w = wave_id(), lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * kMergeWaves + w;
  if (t >= W.n_tiles) return;  // the whole wave; no block-wide barrier below
  const int64_t base = t * 64;
  const uint64_t M = W.start_bits[t];
  const uint64_t Mn = t + 1 < W.n_tiles ? W.start_bits[t + 1] : ~0ull;
  const uint64_t lo = bpe_upto(M, lane), hi = bpe_above(M, lane);
  const int ws = lo ? 63 - __builtin_clzll(lo) : -1;
  const int we = hi ? __builtin_ctzll(hi) : ((Mn & 1) ? 64 : 65);  // 65: past the tile
  const bool in = base + lane < W.n_bytes && ws >= 0 && we <= 64;
  merge_window(T, W, base, in, ws, we, slots[w]);
  // the straddler: the tile's last start, if its word does not end with the tile
  if (!M || (Mn & 1)) return;
  const int js = 63 - __builtin_clzll(M);
  if (base + js >= W.n_bytes) return;
  const int len = Mn ? 64 - js + __builtin_ctzll(Mn) : 129;
  if (len <= 64) {
    merge_window(T, W, base + js, lane < len, 0, len, slots[w]);
  } else if (lane == 0) {
    const unsigned long long k = atomicAdd(W.long_count, 1ull);
    if ((int64_t)k < W.long_cap) W.long_list[k] = base + js;
  }
}

__device__ inline uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

// the first pre-token start after byte x0 (x0 starts one): the word's end
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
      const uint32_t l32 = (uint32_t)__shfl((int)(uint32_t)m, f, 64);
      const uint32_t h32 = (uint32_t)__shfl((int)(uint32_t)(m >> 32), f, 64);
      const uint64_t mf = (uint64_t)h32 << 32 | l32;
      return (w0 + f) * 64 + __builtin_ctzll(mf);
    }
  }
}

__global__ void __launch_bounds__(64) bpe_merge_long_kernel(BpeTables T, BpeWork W) {
  __shared__ uint32_t ids[kBpeMaxWord], rk[kBpeMaxWord], mg[kBpeMaxWord];
  __shared__ uint16_t ps[kBpeMaxWord];
  const int lane = lane_id();
  unsigned long long count = *W.long_count;
  if (count > (unsigned long long)W.long_cap) count = (unsigned long long)W.long_cap;
  for (int64_t i = blockIdx.x; i < (int64_t)count; i += gridDim.x) {
    const int64_t x0 = W.long_list[i];
    int64_t end = word_end(W, x0);
    end = end < W.n_bytes ? end : W.n_bytes;
    for (int64_t a = x0; a < end; a += kBpeMaxWord) {
      int n = (int)(end - a < kBpeMaxWord ? end - a : kBpeMaxWord);
      wave_sync();
      for (int k = lane; k < n; k += 64) {
        ids[k] = (uint32_t)T.byte_id[W.text[a + k]];
        ps[k] = (uint16_t)k;
      }
      wave_sync();
      for (;;) {
        uint32_t best = kBpeNoRank;
        for (int k = lane; k < n; k += 64) {
          uint32_t r = kBpeNoRank, m = 0;
          if (k + 1 < n) probe(T, ids[k], ids[k + 1], &r, &m);
          rk[k] = r;
          mg[k] = m;
          best = r < best ? r : best;
        }
        best = wave_min_u32(best);
        if (best == kBpeNoRank) break;
        wave_sync();
        int out = 0, carry_cnt = 0;
        bool carry_run = false, prev_sel = false;
        for (int k0 = 0; k0 < n; k0 += 64) {
          const int k = k0 + lane;
          const bool in = k < n;
          const bool cand = in && rk[k] == best;
          const uint32_t my_id = in ? ids[k] : 0u, my_mg = in ? mg[k] : 0u;
          const uint16_t my_ps = in ? ps[k] : (uint16_t)0;
          const uint64_t C = ballot(cand);
          uint64_t RS = C & ~(C << 1);
          if (carry_run) RS &= ~1ull;  // the run of the stride before goes on
          const uint64_t rs_lo = bpe_upto(RS, lane);
          const uint64_t below = C & ((1ull << lane) - 1);
          int before;
          if (rs_lo) {
            const int s = 63 - __builtin_clzll(rs_lo);
            before = __popcll(below & ~((1ull << s) - 1));
          } else {
            before = __popcll(below) + carry_cnt;
          }
          const bool sel = cand && !(before & 1);
          const uint64_t SEL = ballot(sel);
          const bool left_sel = lane == 0 ? prev_sel : (bool)((SEL >> (lane - 1)) & 1);
          const bool keep = in && !left_sel;
          const uint64_t K = ballot(keep);
          const int last_before = __builtin_amdgcn_readlane(before, 63);
          wave_sync();  // the stride's reads are done before its (lower or equal) slots change
          if (keep) {
            const int d = out + (int)popc_below(K);
            ids[d] = sel ? my_mg : my_id;
            ps[d] = my_ps;
          }
          out += __popcll(K);
          carry_run = (C >> 63) & 1;
          carry_cnt = carry_run ? (last_before + 1) & 1 : 0;
          prev_sel = (SEL >> 63) & 1;
        }
        n = out;
        wave_sync();
      }
      for (int k = lane; k < n; k += 64) {
        const int64_t x = a + ps[k];
        W.sym[x] = (int32_t)ids[k];
        atomicOr(reinterpret_cast<unsigned long long*>(W.alive_bits + (x >> 6)), 1ull << (x & 63));
      }
    }
  }
}

}  // namespace

hipError_t bpe_launch_merge(const BpeTables& T, const BpeWork& W, hipStream_t st) {
  hipLaunchKernelGGL(bpe_merge_tile_kernel, dim3((unsigned)((W.n_tiles + kMergeWaves - 1) / kMergeWaves)),
                     dim3(64 * kMergeWaves), 0, st, T, W);
  const int64_t g = W.long_cap < kLongGrid ? W.long_cap : kLongGrid;
  hipLaunchKernelGGL(bpe_merge_long_kernel, dim3((unsigned)(g > 0 ? g : 1)), dim3(64), 0, st, T, W);
  return hipGetLastError();
}

}  // namespace lddl
