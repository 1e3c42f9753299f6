// T5 span corruption, the device side of t5_corrupt.hip: the kernel's arguments,
// the LDS of a wave, the fixed-point counts (shared with the host's lddl_t5_lengths), the token
// at a position of a block, one digit of the radix select and the bisection of a start table.
// include/lddl_amd.h states the semantics. The translation unit gets its own copy.
#pragma once
#include "blocks_dev.h"   // kBlkLdsSents
#include "collate_dev.h"  // mask_draw, kEncWaves

namespace lddl {
namespace {

constexpr int kT5MaxSpans = LDDL_T5_MAX_SPANS;
constexpr int kT5Bins = 256;  // one 8-bit digit of a 24-bit key
static_assert(kT5MaxSpans == 256 && kT5Bins == 4 * 64,
              "t5_locate takes eight steps and a lane scans four bins");

struct T5Args {
  const int32_t* ids;
  const int64_t* sent_off;
  const int64_t* P;    // piece_off[n_sent + 1]
  const uint8_t* sep;  // [n_sent]
  const int64_t* block_sent;
  const int64_t* rows;  // nullable: identity
  int32_t B, L, in_len, tgt_len, dq, iq, n_sentinels;
  int64_t sentinel_first, eos, pad, dec_start, ignore_index;
  MaskDraw draw;  // seed and counter; the rest is unread
  int64_t* input_ids;
  int64_t* attention_mask;
  int64_t* labels;
  int64_t* decoder_input_ids;
  int64_t* src_lengths;
  int64_t* tgt_lengths;
};

// One wave's LDS, 5,136 bytes: the two histograms of a select pass (noise, non-noise), the
// block's sentence table, and the first items of the non-noise (A) and noise (Bn) segments.
struct T5Wave {
  alignas(16) uint32_t hist[2][kT5Bins];
  int32_t rel[kBlkLdsSents + 1];
  int32_t A[kT5MaxSpans + 1];
  int32_t Bn[kT5MaxSpans + 1];
};

// N noise tokens in k spans of a row of n tokens; dq, iq in 16.16 fixed point
__host__ __device__ inline void t5_counts(int64_t n, int64_t dq, int64_t iq, int64_t n_sentinels,
                                          int32_t* N, int32_t* k) {
  *N = *k = 0;
  if (n < 2) return;
  int64_t a = (n * dq + 32768) >> 16;
  a = a < 1 ? 1 : (a > n - 1 ? n - 1 : a);
  int64_t hi = a < n - a ? a : n - a;
  hi = hi < n_sentinels ? hi : n_sentinels;
  int64_t c = (a * iq + 32768) >> 16;
  c = c < 1 ? 1 : (c > hi ? hi : c);
  *N = (int32_t)a;
  *k = (int32_t)c;
}

// The block of a row as the wave staged it: rel[j] = P[s0 + j] - p0 for j <= U in LDS
struct T5Block {
  const int32_t* rel;
  int32_t U;
  int64_t s0, s1, p0;
};

// The token at position q, 0 <= q < n, of the block: blocks_kernel's lookup. The largest s with
// rel[s] <= q by bisection (the sentence after it starts past q, so empty sentences are
// skipped), in global P past the staged table; the offset is a kept piece or the separator.
__device__ inline int64_t t5_token(const T5Args& A, const T5Block& K, int32_t q) {
  int64_t s;
  int32_t rs, rn;
  if (q < K.rel[K.U]) {
    int32_t lo = 0, hi = K.U;
    while (hi - lo > 1) {
      const int32_t mid = (lo + hi) >> 1;
      if (K.rel[mid] <= q) lo = mid;
      else hi = mid;
    }
    s = K.s0 + lo;
    rs = K.rel[lo];
    rn = K.rel[lo + 1];
  } else {
    int64_t lo = K.s0 + K.U, hi = K.s1;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (A.P[mid] - K.p0 <= q) lo = mid;
      else hi = mid;
    }
    s = lo;
    rs = (int32_t)(A.P[lo] - K.p0);
    rn = (int32_t)(A.P[lo + 1] - K.p0);
  }
  const int32_t o = q - rs, kept = rn - rs - A.sep[s];
  return o < kept ? (int64_t)A.ids[A.sent_off[s] + o] : A.eos;
}

// One digit of the select, EVERY lane calls it: bins = the histogram of this digit over the
// keys that match the prefix, 1 <= want <= their number. Returns the digit whose bin holds the
// key of rank `want` (1-based) and turns `want` into the rank inside that bin. A lane sums four
// bins, the wave scans the sums, the first lane whose inclusive sum reaches `want` walks its
// four.
__device__ inline uint32_t t5_pick(const uint32_t* bins, int lane, uint32_t& want) {
  const uint4 c = *reinterpret_cast<const uint4*>(bins + 4 * lane);
  const uint32_t s = c.x + c.y + c.z + c.w;
  const uint32_t incl = wave_incl_scan(s);
  const uint64_t ge = ballot(incl >= want);
  const int src = ge ? __builtin_ctzll(ge) : 63;
  uint32_t w = want - (incl - s), d = 0;  // meaningful in lane src only
  if (w > c.x) {
    w -= c.x;
    d = 1;
    if (w > c.y) {
      w -= c.y;
      d = 2;
      if (w > c.z) {
        w -= c.z;
        d = 3;
      }
    }
  }
  want = __shfl(w, src, 64);
  return __shfl(4u * lane + d, src, 64);
}

// The segment that holds slot x of a compacted row: the largest g in [0, k) with tab[g] + g <=
// x, for tab[0] = 0 <= x and k <= kT5MaxSpans. Segment g and its sentinel take tab[g + 1] -
// tab[g] + 1 slots from slot tab[g] + g on. Eight LDS reads, the same for every lane.
__device__ inline int32_t t5_locate(const int32_t* tab, int32_t k, int32_t x) {
  int32_t g = 0;
#pragma unroll
  for (int step = kT5MaxSpans / 2; step >= 1; step >>= 1)
    if (g + step < k && tab[g + step] + g + step <= x) g += step;
  return g;
}

}  // namespace
}  // namespace lddl
