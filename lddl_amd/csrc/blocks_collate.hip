// The RoBERTa collate (include/lddl_amd.h states the semantics): output row i is
// block rows[i] of lddl_blocks_plan, a run of ragged sentences read in place from the token
// table: bos, the kept pieces of the block's sentences with eos behind a document's last one,
// eos, pad. One wave per row, kEncWaves rows per workgroup, no block-wide barrier.
//
//   table    the wave stages rel[j] = P[s0 + j] - P[s0], j <= min(S, kBlkLdsSents), in LDS
//   slots    64 slots a step, lane = slot x: position q = x - 1 of the block; the lane bisects
//            rel for the largest s with rel[s] <= q (the sentence after it starts past q, so
//            empty sentences are skipped); past the staged table it bisects global P. The
//            offset q - rel[s] is a kept piece (one load at sent_off[s] + offset) or, at
//            c(s) - 1 of a sentence with sep, the separator
//   masking  per token: the slot's own draw; word mode: heads (first kept piece of a sentence,
//            or no continuation id) into span_masked, the one word loop of this kernel (n = 1
//            is whole-word masking); 80 / 10 / 10 by mask_apply
//
// Every output element is written exactly once; every lane reaches the ballot and the scan of
// span_masked, the tail of the row is predicated.
#include "blocks_dev.h"
#include "collate_host.h"  // span_draw_of; collate_dev.h, span_dev.h
#include "common.h"
#include "ctx.h"

namespace lddl {
namespace {

struct BlocksArgs {
  const int32_t* ids;
  const int64_t* sent_off;
  const int64_t* P;    // piece_off[n_sent + 1]
  const uint8_t* sep;  // [n_sent]
  const int64_t* block_sent;
  const int64_t* rows;  // nullable: identity
  int32_t B, L;
  int64_t* input_ids;
  int64_t* attention_mask;
  int64_t* second;  // special_tokens_mask (kPlain) or labels
  int64_t bos, eos, pad;
  MaskDraw draw;
  ContBits cont;
  SpanDraw span;
};

template <int MODE>
__global__ void __launch_bounds__(64 * kEncWaves) blocks_kernel(BlocksArgs A) {
  __shared__ int32_t tables[kEncWaves][kBlkLdsSents + 1];
  const int w = wave_id(), lane = lane_id();
  const int32_t b = blockIdx.x * kEncWaves + w;
  if (b >= A.B) return;  // the whole wave; no block-wide barrier below
  int32_t* rel = tables[w];
  const int64_t k = A.rows ? A.rows[b] : (int64_t)b;
  const int64_t s0 = A.block_sent[k], s1 = A.block_sent[k + 1];
  const int64_t S = s1 - s0, p0 = A.P[s0];
  const int32_t T = A.L - 2;
  const int64_t m64 = A.P[s1] - p0;  // the plan keeps a block within T
  const int32_t M = (int32_t)(m64 < 0 ? 0 : (m64 < T ? m64 : T));
  const int32_t U = (int32_t)(S < kBlkLdsSents ? (S < 0 ? 0 : S) : kBlkLdsSents);
  for (int32_t j = lane; j <= U; j += 64) {
    const int64_t r = A.P[s0 + j] - p0;
    rel[j] = (int32_t)(r < T + 1 ? r : T + 1);  // every q is below T: the clip orders the same
  }
  wave_sync();
  const int64_t row = (int64_t)b * A.L;
  int32_t words_before = 0;  // the state of span_masked between the row's windows
  uint32_t carry_max = 0;
  for (int32_t x0 = 0; x0 < A.L; x0 += 64) {
    const int32_t x = x0 + lane, q = x - 1;
    const bool in = x < A.L;
    int64_t id = x == 0 ? A.bos : (q == M ? A.eos : A.pad);
    bool special = true, first = false;
    if (in && x >= 1 && q < M) {
      int64_t s;
      int32_t rs, rn;  // rel of the sentence and of the one after it
      if (q < rel[U]) {  // rel[0] = 0 <= q
        int32_t lo = 0, hi = U;
        while (hi - lo > 1) {
          const int32_t mid = (lo + hi) >> 1;
          if (rel[mid] <= q) lo = mid;
          else hi = mid;
        }
        s = s0 + lo;
        rs = rel[lo];
        rn = rel[lo + 1];
      } else {  // a block of more than kBlkLdsSents sentences: P[s0 + U] - p0 <= q < M
        int64_t lo = s0 + U, hi = s1;
        while (hi - lo > 1) {
          const int64_t mid = lo + (hi - lo) / 2;
          if (A.P[mid] - p0 <= q) lo = mid;
          else hi = mid;
        }
        s = lo;
        rs = (int32_t)(A.P[lo] - p0);
        rn = (int32_t)(A.P[lo + 1] - p0);
      }
      const int32_t o = q - rs, kept = rn - rs - A.sep[s];
      id = A.eos;  // the separator, unless the offset is a kept piece
      if (o < kept) {
        id = A.ids[A.sent_off[s] + o];
        special = false;
        first = o == 0;
      }
    }
    int64_t out = id, second = special ? 1 : 0;
    if constexpr (MODE != kPlain) {
      const uint4 r = mask_draw(A.draw, row + x);
      bool m;
      if constexpr (MODE == kFusedSpan)
        m = span_masked(A.span, A.draw.counter,
                        in && !special && (first || !cont_id(A.cont, id)), r, row + x,
                        words_before, carry_max);
      else
        m = u01(r.x) < A.draw.p;
      out = mask_apply(A.draw, r, !special && m, id, &second);
    }
    if (in) {
      A.input_ids[row + x] = out;
      A.attention_mask[row + x] = q <= M ? 1 : 0;
      A.second[row + x] = second;
    }
  }
}

template <int MODE>
int launch(const BlocksArgs& A, void* stream) {
  hipLaunchKernelGGL(blocks_kernel<MODE>, dim3((unsigned)((A.B + kEncWaves - 1) / kEncWaves)),
                     dim3(64 * kEncWaves), 0, as_stream(stream), A);
  LDDL_HIP(hipGetLastError());
  return 0;
}

// the refusals the two entry points share; 1 = nothing to do
int blocks_check(const int32_t* d_ids, const int64_t* d_sent_off, const int64_t* d_piece_off,
                 const uint8_t* d_sent_sep, const int64_t* d_block_sent, int32_t batch,
                 int32_t seq_len, const void* o0, const void* o1, const void* o2) {
  if (seq_len < 3 || seq_len > (1 << 24))
    LDDL_FAIL(-1, "seq_len %d: a row holds bos, a piece and eos at least, 2^24 slots at most",
              seq_len);
  if (batch <= 0) return 1;
  if (!d_ids || !d_sent_off || !d_piece_off || !d_sent_sep || !d_block_sent)
    LDDL_FAIL(-1, "null token table or plan");
  if (!o0 || !o1 || !o2) LDDL_FAIL(-1, "null output");
  return 0;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_collate_blocks(void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                                   const int64_t* d_piece_off, const uint8_t* d_sent_sep,
                                   const int64_t* d_block_sent, const int64_t* d_rows,
                                   int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                                   int64_t* d_attention_mask, int64_t* d_special_tokens_mask,
                                   int64_t bos_id, int64_t eos_id, int64_t pad_id) {
  const int st = blocks_check(d_ids, d_sent_off, d_piece_off, d_sent_sep, d_block_sent, batch,
                              seq_len, d_input_ids, d_attention_mask, d_special_tokens_mask);
  if (st) return st < 0 ? st : 0;
  const BlocksArgs A{d_ids, d_sent_off, d_piece_off, d_sent_sep, d_block_sent, d_rows, batch,
                     seq_len, d_input_ids, d_attention_mask, d_special_tokens_mask, bos_id,
                     eos_id, pad_id, {}, {}, {}};
  return launch<kPlain>(A, stream);
}

extern "C" int lddl_collate_blocks_masked(
    const uint32_t* d_cont_bits, int64_t n_ids, void* stream, const int32_t* d_ids,
    const int64_t* d_sent_off, const int64_t* d_piece_off, const uint8_t* d_sent_sep,
    const int64_t* d_block_sent, const int64_t* d_rows, int32_t batch, int32_t seq_len,
    int64_t* d_input_ids, int64_t* d_attention_mask, int64_t* d_labels, int64_t bos_id,
    int64_t eos_id, int64_t pad_id, int64_t mask_id, float mlm_probability, int64_t ignore_index,
    int64_t vocab_len, uint64_t seed, uint64_t counter, const lddl_span_params* params) {
  SpanDraw S{};
  if (params && span_draw_of(params, seed, &S)) return -1;
  if (!(mlm_probability >= 0.f && mlm_probability <= 1.f))
    LDDL_FAIL(-1, "mlm_probability must lie in [0, 1]");
  if (vocab_len < 1 || vocab_len > (int64_t)1 << 32) LDDL_FAIL(-1, "vocab_len outside [1, 2^32]");
  if (n_ids < 1 || n_ids > INT32_MAX) LDDL_FAIL(-1, "n_ids outside [1, 2^31)");
  const int st = blocks_check(d_ids, d_sent_off, d_piece_off, d_sent_sep, d_block_sent, batch,
                              seq_len, d_input_ids, d_attention_mask, d_labels);
  if (st) return st < 0 ? st : 0;
  if (params && !d_cont_bits) LDDL_FAIL(-1, "null continuation bitmap");
  const BlocksArgs A{d_ids, d_sent_off, d_piece_off, d_sent_sep, d_block_sent, d_rows, batch,
                     seq_len, d_input_ids, d_attention_mask, d_labels, bos_id, eos_id, pad_id,
                     MaskDraw{mlm_probability, ignore_index, mask_id, vocab_len, seed, counter},
                     ContBits{d_cont_bits, (int32_t)n_ids}, S};
  return params ? launch<kFusedSpan>(A, stream) : launch<kFused>(A, stream);
}
