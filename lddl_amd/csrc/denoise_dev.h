// BART denoising, the device side of denoise.hip: the kernel's arguments, the
// length draw of a span, the bisection of a position table in LDS and the source of a piece.
// The translation unit gets its own copy (anonymous namespace).
#pragma once
#include "collate_dev.h"  // u01, mask_draw's counter layout, ContBits
#include "denoise_shape.h"

namespace lddl {
namespace {

constexpr int kDenoiseMaxN = 16;

struct DenoiseDraw {
  uint64_t seed2;  // seed ^ LDDL_SPAN_SEED_XOR: the key of the length draw
  float p_start;
  float cum[kDenoiseMaxN];  // cum[k] = P(len <= k) for k < n, 1 from there on
};

struct DenoiseArgs {
  const int32_t* ids;           // ctx.tokenize's output, read in place
  const int64_t* sent_off;      // sentence s: ids[sent_off[s] ..) holds sent_len[s] & kLenMask pieces
  const int32_t* sent_len;
  const int64_t* doc_sent_off;  // a document is a sample
  const int64_t* rows;          // nullable: identity
  int32_t B, L, draw_stride;
  int64_t* input_ids;
  int64_t* attention_mask;
  int64_t* decoder_input_ids;
  int64_t* labels;
  int32_t* src_lengths;
  int64_t bos, eos, pad, mask_id, dec_start, ignore_index, vocab_len;
  uint64_t seed, sent_seed, counter;  // sent_seed = seed ^ LDDL_DENOISE_SENT_XOR
  float permute_p, random_ratio;
  ContBits cont;
  DenoiseDraw draw;
};

// the collates' Philox call: the flat index low and high, the counter low and high, key = seed
__device__ inline uint4 denoise_draw(uint64_t key, uint64_t counter, int64_t flat) {
  return Philox::gen(make_uint4((uint32_t)flat, (uint32_t)(flat >> 32), (uint32_t)counter,
                                (uint32_t)(counter >> 32)),
                     make_uint2((uint32_t)key, (uint32_t)(key >> 32)));
}

// len = #{k in [0, n) : u >= cum[k]} in 0 .. n; the entries from n on are 1 > u
__device__ inline int32_t denoise_len(const DenoiseDraw& D, uint64_t counter, int64_t flat) {
  const float u = u01(denoise_draw(D.seed2, counter, flat).x);
  int32_t len = 0;
#pragma unroll
  for (int k = 0; k < kDenoiseMaxN; ++k) len += u >= D.cum[k] ? 1 : 0;
  return len;
}

// The largest k in [0, U) with tab[k] <= x, for 0 <= x < tab[U] and U <= kDenoiseUnits: the unit
// that holds position x of a table of first positions. A unit of length 0 shares its entry with
// the next one and is never the answer. Eight LDS reads, the same for every lane.
__device__ inline int32_t denoise_locate(const int32_t* tab, int32_t U, int32_t x) {
  int32_t k = 0;
#pragma unroll
  for (int step = kDenoiseUnits / 2; step >= 1; step >>= 1)
    if (k + step < U && tab[k + step] <= x) k += step;
  return k;
}

// Piece `off` of unit u of the sample whose sentences start at s0 (S of them): its id and
// whether it is the first piece of its sentence. A unit below the last is sentence s0 + u. The
// tail unit is the sentences from s0 + kDenoiseUnits - 1 on in their order, which the lane
// walks: off lies inside the unit, so the walk ends at or before the sample's last sentence.
__device__ inline int32_t denoise_piece(const DenoiseArgs& A, int64_t s0, int64_t S, int32_t u,
                                        int32_t off, bool* first) {
  int64_t s = s0 + u;
  if (u == kDenoiseUnits - 1) {
    for (; s + 1 < s0 + S; ++s) {
      const int32_t l = A.sent_len[s] & kLenMask;
      if (off < l) break;
      off -= l;
    }
  }
  *first = off == 0;
  return A.ids[A.sent_off[s] + off];
}

}  // namespace
}  // namespace lddl
