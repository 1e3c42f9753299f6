// The GPT rows (include/lddl_amd.h states the semantics): output row i is the
// window of L + 1 stream positions from rows[i] * L of lddl_stream_plan's stream, gathered from
// the token table in place: input_ids, the shifted labels, position_ids, sequence_ids, and
// cu_seqlens for the batch. A GPT batch is few long rows, so the grid is (tiles of a row) x
// (batch rows): a workgroup of kStrThreads takes kStrTile slots.
//
//   places   every wave finds, by wave_place's 64-way search of Q, the places of the row's first
//            position (for sequence_ids), of the tile's first and of its last position (the
//            four waves search side by side, so no barrier stands before the staging)
//   stage    thread k < U = min(places of the tile, kStrLdsDocs) stages place p_first + k in
//            LDS: rel[k] = Q - g0 and the document's StreamDoc (sentence range, first token's
//            rank, t, the FIM layout and cuts): one Philox call per document per tile. One
//            barrier.
//   slots    a thread owns 4 consecutive slots and resolves 5 stream positions, the fifth for
//            the last label. Place: bisection of rel in LDS, in global Q past the staged
//            table. Offset in the document -> terminator, sentinel or source index by
//            stream_map. Sentence: bisection of sent_tok_off over the document's range. The
//            thread carries the place and the sentence of its last hit and tests them first.
//   stores   two 16-byte vectors per thread and output, consecutive over the workgroup; a
//            thread at the row's ragged end stores its slots one by one.
//
// Every output element is written exactly once. No atomics, no scratch.
#include "common.h"
#include "ctx.h"
#include "scan.h"  // block_excl_scan
#include "stream_dev.h"

namespace lddl {
namespace {

struct RowsArgs {
  StreamSrc S;
  const int32_t* ids;
  const int64_t* sent_off;
  const int64_t* Q;     // doc_off[n_doc + 1]
  const int64_t* rows;  // nullable: identity
  int32_t B, L, tiles, eod_mask_loss, reset_position_ids;
  int64_t eos, pre, mid, suf, ignore_index;
  int64_t* input_ids;
  int64_t* labels;
  int64_t* position_ids;
  int64_t* sequence_ids;
};

// 16 bytes at the alignment of an element: row i starts at element i * L, which may be odd
typedef int64_t i64x2 __attribute__((ext_vector_type(2), aligned(8)));

__device__ inline void store4(int64_t* p, const int64_t (&v)[kStrItems], int32_t n) {
  if (n >= kStrItems) {
    i64x2 lo, hi;
    lo.x = v[0], lo.y = v[1], hi.x = v[2], hi.y = v[3];
    *reinterpret_cast<i64x2*>(p) = lo;
    *reinterpret_cast<i64x2*>(p + 2) = hi;
  } else {
#pragma unroll
    for (int k = 0; k < kStrItems - 1; ++k)
      if (k < n) p[k] = v[k];
  }
}

// the rows of the plan, from its last offset
__device__ inline int64_t plan_rows(const int64_t* Q, int64_t n_doc, int32_t L) {
  const int64_t total = Q[n_doc];
  return total > 0 ? (total - 1) / L : 0;
}

__global__ void __launch_bounds__(kStrThreads) stream_rows_kernel(RowsArgs A) {
  __shared__ int32_t rel[kStrLdsDocs];
  __shared__ StreamDoc docs[kStrLdsDocs];
  const int64_t* Q = A.Q;
  const int64_t n_doc = A.S.n_doc;
  const int32_t tile = blockIdx.x % A.tiles, i = blockIdx.x / A.tiles;
  const int64_t n_rows = plan_rows(Q, n_doc, A.L);
  if (n_rows < 1) return;  // the whole workgroup: a plan without a row
  const int64_t r = clamp_to(A.rows ? A.rows[i] : (int64_t)i, n_rows - 1);
  const int32_t y0 = tile * kStrTile;
  const int32_t n = A.L - y0 < kStrTile ? A.L - y0 : kStrTile;
  const int64_t row0 = r * A.L, g0 = row0 + y0;
  // positions g0 .. g0 + n are below Q[n_doc]: g0 + n <= n_rows * L <= Q[n_doc] - 1
  const int64_t p_row = wave_place(Q, 0, n_doc, row0);
  const int64_t p_first = tile == 0 ? p_row : wave_place(Q, p_row, n_doc, g0);
  // a place takes a position at least: Q[p_first + 1 + n] > g0 + n
  const int64_t far = p_first + 1 + n;
  const int64_t p_last = wave_place(Q, p_first, far < n_doc ? far : n_doc, g0 + n);
  const int64_t span = p_last - p_first + 1;
  const int32_t U = (int32_t)(span < kStrLdsDocs ? span : kStrLdsDocs);
  const int64_t off0 = g0 - Q[p_first];  // of g0 in the first place, >= 0
  if ((int32_t)threadIdx.x < U) {
    const int64_t j = p_first + threadIdx.x;
    docs[threadIdx.x] = stream_doc(A.S, j);
    rel[threadIdx.x] = threadIdx.x == 0 ? 0 : (int32_t)(Q[j] - g0);  // in (0, n] behind the first
  }
  __syncthreads();

  const int32_t x0 = (int32_t)threadIdx.x * kStrItems;
  const int32_t left = n - x0;  // the thread's slots inside the row
  if (left <= 0) return;        // (no barrier below)
  int64_t in[kStrItems], lab[kStrItems], pos[kStrItems], sid[kStrItems];
  bool term[kStrItems];
  StreamDoc cur = docs[0];
  int64_t cur_rel = -off0, cur_place = p_first;  // the place's first position, minus g0
  bool have = false;
  int64_t cs_lo = 0, cs_hi = 0, cs_at = 0;  // the carried sentence: ranks [cs_lo, cs_hi) at ids + cs_at
#pragma unroll
  for (int k = 0; k <= kStrItems; ++k) {
    const int32_t x = x0 + k;
    if (x > n) continue;
    if (!have || x - cur_rel >= cur.cost()) {
      int32_t lo = 0, hi = U;  // rel[0] = 0 <= x
      while (hi - lo > 1) {
        const int32_t m = (lo + hi) >> 1;
        if (rel[m] <= x) lo = m;
        else hi = m;
      }
      cur = docs[lo];
      cur_rel = lo == 0 ? -off0 : (int64_t)rel[lo];
      cur_place = p_first + lo;
      if (x - cur_rel >= cur.cost()) {  // past the staged table: Q[p_first + U - 1] <= g0 + x
        cur_place = lane_place(Q, p_first + U - 1, p_last + 1, g0 + x);
        cur = stream_doc(A.S, cur_place);
        cur_rel = Q[cur_place] - g0;
      }
      have = true;
    }
    const int32_t o = (int32_t)(x - cur_rel);
    int32_t q;
    const int what = stream_map(cur, o, &q);
    int64_t tok = what == kTokEos ? A.eos : (what == kTokPre ? A.pre : (what == kTokSuf ? A.suf : A.mid));
    if (what == kTokSource) {
      const int64_t rank = cur.base + q;
      if (rank < cs_lo || rank >= cs_hi) {
        int64_t lo = cur.s0, hi = cur.s0 + cur.ns;  // sto[lo] <= rank < sto[hi]
        while (hi - lo > 1) {
          const int64_t m = lo + (hi - lo) / 2;
          if (A.S.sto[m] <= rank) lo = m;
          else hi = m;
        }
        cs_lo = A.S.sto[lo];
        cs_hi = A.S.sto[lo + 1];
        cs_at = A.sent_off[lo];
      }
      tok = A.ids[cs_at + (rank - cs_lo)];
    }
    if (k > 0) lab[k - 1] = A.eod_mask_loss && term[k - 1] ? A.ignore_index : tok;
    if (k < kStrItems) {
      const int64_t y = y0 + x;
      in[k] = tok;
      term[k] = what == kTokEos;
      pos[k] = A.reset_position_ids && o < y ? (int64_t)o : y;
      sid[k] = cur_place - p_row;
    }
  }
  const int64_t at = (int64_t)i * A.L + y0 + x0;
  store4(A.input_ids + at, in, left);
  store4(A.labels + at, lab, left);
  store4(A.position_ids + at, pos, left);
  store4(A.sequence_ids + at, sid, left);
}

struct CuArgs {
  const int64_t* Q;
  int64_t n_doc;
  const int64_t* rows;
  int32_t B, L, max_seqs;
  int32_t* cu;
  int32_t* n_seqs;
};

// One workgroup. A sequence starts at slot 0 of a row and at every slot behind a terminator,
// which is a position Q[j] inside (row0, row0 + L - 1]: two bisections count a row's starts.
__global__ void __launch_bounds__(kScanThreads) stream_cu_kernel(CuArgs A) {
  __shared__ int64_t s_base[kScanThreads], s_place[kScanThreads], s_row0[kScanThreads];
  __shared__ int32_t s_cnt[kScanThreads];
  const int64_t n_rows = plan_rows(A.Q, A.n_doc, A.L);
  const int w = wave_id(), lane = lane_id();
  int64_t carry = 0;
  for (int32_t b0 = 0; b0 < A.B; b0 += kScanThreads) {
    const int32_t i = b0 + (int32_t)threadIdx.x;
    int64_t cnt = 0, row0 = 0, p0 = 0;
    if (i < A.B && n_rows >= 1) {
      row0 = clamp_to(A.rows ? A.rows[i] : (int64_t)i, n_rows - 1) * A.L;
      p0 = lane_place(A.Q, 0, A.n_doc, row0);
      cnt = 1 + lane_place(A.Q, p0, A.n_doc, row0 + A.L - 1) - p0;
    }
    int64_t tot;
    s_base[threadIdx.x] = carry + block_excl_scan(cnt, &tot);
    s_place[threadIdx.x] = p0;
    s_row0[threadIdx.x] = row0;
    s_cnt[threadIdx.x] = (int32_t)cnt;
    __syncthreads();
    const int32_t nb = A.B - b0 < kScanThreads ? A.B - b0 : kScanThreads;
    for (int32_t v = w; v < nb; v += kScanThreads / 64) {  // a wave per row, lane = start
      const int64_t first = (int64_t)(b0 + v) * A.L;
      for (int32_t k = lane; k < s_cnt[v]; k += 64) {
        const int64_t at = s_base[v] + k;
        if (at < A.max_seqs)
          A.cu[at] = (int32_t)(first + (k == 0 ? 0 : A.Q[s_place[v] + k] - s_row0[v]));
      }
    }
    carry += tot;
    __syncthreads();
  }
  const int64_t end = (int64_t)A.B * A.L;
  for (int64_t at = (carry < A.max_seqs ? carry : A.max_seqs) + threadIdx.x; at <= A.max_seqs;
       at += kScanThreads)
    A.cu[at] = (int32_t)end;
  if (threadIdx.x == 0) A.n_seqs[0] = (int32_t)carry;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_stream_rows(void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                                int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                                const int64_t* d_doc_order, const int64_t* d_sent_tok_off,
                                const int64_t* d_doc_off, const int64_t* d_rows, int32_t batch,
                                int32_t seq_len, int32_t fim_q, int32_t spm_q, uint64_t seed,
                                uint64_t counter, int64_t eos_id, int64_t fim_prefix_id,
                                int64_t fim_middle_id, int64_t fim_suffix_id,
                                int32_t eod_mask_loss, int32_t reset_position_ids,
                                int64_t ignore_index, int64_t* d_input_ids, int64_t* d_labels,
                                int64_t* d_position_ids, int64_t* d_sequence_ids) {
  if (seq_len < 1 || seq_len > (1 << 20)) LDDL_FAIL(-1, "seq_len %d is outside [1, 2^20]", seq_len);
  if (fim_q < 0 || fim_q > 65536 || spm_q < 0 || spm_q > 65536)
    LDDL_FAIL(-1, "fim_q %d or spm_q %d is outside [0, 65536]", fim_q, spm_q);
  if (n_sent < 0 || n_doc < 0 || batch < 0) LDDL_FAIL(-1, "negative size");
  if (eos_id < 0) LDDL_FAIL(-1, "negative eos_id");
  if (fim_q > 0 && (fim_prefix_id < 0 || fim_middle_id < 0 || fim_suffix_id < 0))
    LDDL_FAIL(-1, "fim_q > 0 needs fim_prefix_id, fim_middle_id and fim_suffix_id");
  if (!d_sent_tok_off || !d_doc_off) LDDL_FAIL(-1, "null plan");
  if (n_sent > 0 && (!d_ids || !d_sent_off)) LDDL_FAIL(-1, "null token table");
  if (n_doc > 0 && !d_doc_sent_off) LDDL_FAIL(-1, "null doc_sent_off");
  if (batch > 0 && (!d_input_ids || !d_labels || !d_position_ids || !d_sequence_ids))
    LDDL_FAIL(-1, "null output");
  const int64_t tiles = (seq_len + kStrTile - 1) / kStrTile;
  if (batch * tiles > INT32_MAX) LDDL_FAIL(-1, "batch %d at seq_len %d: too many tiles", batch, seq_len);
  if (batch == 0 || n_doc == 0) return 0;  // no document, no row
  RowsArgs A{};
  A.S = StreamSrc{d_doc_sent_off, d_doc_order, d_sent_tok_off, n_sent, n_doc,
                  (uint32_t)fim_q, (uint32_t)spm_q, seed, counter};
  A.ids = d_ids;
  A.sent_off = d_sent_off;
  A.Q = d_doc_off;
  A.rows = d_rows;
  A.B = batch;
  A.L = seq_len;
  A.tiles = (int32_t)tiles;
  A.eod_mask_loss = eod_mask_loss != 0;
  A.reset_position_ids = reset_position_ids != 0;
  A.eos = eos_id;
  A.pre = fim_prefix_id;
  A.mid = fim_middle_id;
  A.suf = fim_suffix_id;
  A.ignore_index = ignore_index;
  A.input_ids = d_input_ids;
  A.labels = d_labels;
  A.position_ids = d_position_ids;
  A.sequence_ids = d_sequence_ids;
  hipLaunchKernelGGL(stream_rows_kernel, dim3((unsigned)(batch * tiles)), dim3(kStrThreads), 0,
                     as_stream(stream), A);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_stream_cu_seqlens(void* stream, const int64_t* d_doc_off, int64_t n_doc,
                                      const int64_t* d_rows, int32_t batch, int32_t seq_len,
                                      int32_t max_seqs, int32_t* d_cu_seqlens, int32_t* d_n_seqs) {
  if (seq_len < 1 || seq_len > (1 << 20)) LDDL_FAIL(-1, "seq_len %d is outside [1, 2^20]", seq_len);
  if (n_doc < 0 || batch < 0) LDDL_FAIL(-1, "negative size");
  if (max_seqs < 1) LDDL_FAIL(-1, "max_seqs %d: room for one sequence at least", max_seqs);
  if ((int64_t)batch * seq_len > INT32_MAX)
    LDDL_FAIL(-1, "batch %d at seq_len %d: the flat offsets are int32", batch, seq_len);
  if (!d_doc_off || !d_cu_seqlens || !d_n_seqs) LDDL_FAIL(-1, "null plan or output");
  const CuArgs A{d_doc_off, n_doc, d_rows, batch, seq_len, max_seqs, d_cu_seqlens, d_n_seqs};
  hipLaunchKernelGGL(stream_cu_kernel, dim3(1), dim3(kScanThreads), 0, as_stream(stream), A);
  LDDL_HIP(hipGetLastError());
  return 0;
}
