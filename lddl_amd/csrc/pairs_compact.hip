// Pair stage, compaction (lddl/dask/bert/pretrain.py:89-97, _get_documents): the kept-sentence
// tables, the partitions' kept-document offsets and the dense token buffer.
#include "pairs_plan.h"

namespace lddl {
namespace {

// ---------------------------------------------------------------------------------------------
// Compaction (pretrain.py:89-97): drop sentences with no pieces, then documents with no sentences
// ---------------------------------------------------------------------------------------------
struct KeepSent {
  const int32_t* len;
  __device__ int64_t operator()(int64_t s) const { return (len[s] & kLenMask) > 0; }
};
// both sentence scans in one pass: kept-sentence index and token offset. A dropped sentence has
// no tokens, so the token scan over all sentences, read at the kept ones, is the kept-token scan.
struct SentCounts {
  const int32_t* len;
  __device__ Sum2 operator()(int64_t s) const {
    const int32_t l = len[s] & kLenMask;
    return Sum2{l > 0 ? 1 : 0, l};
  }
};
struct KeepDoc {
  const int64_t* ks_pos;  // exclusive scan of KeepSent, n_sent+1
  const int64_t* doc_sent_off;
  __device__ int64_t operator()(int64_t d) const {
    return ks_pos[doc_sent_off[d + 1]] > ks_pos[doc_sent_off[d]];
  }
};

// kept sentence k = ks_pos[s]: its text start, length and token offset kscan[k] = tok_pos[s]
// (kscan[n_kept] = the total, from thread n_sent)
__global__ void scatter_sentences_kernel(const int64_t* sent_off, const int32_t* sent_len,
                                         int64_t n_sent, const int64_t* ks_pos, const int64_t* tok_pos,
                                         int64_t* ks_start, int32_t* ks_len, int64_t* kscan) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n_sent) return;
  if (s == n_sent) {
    kscan[ks_pos[n_sent]] = tok_pos[n_sent];
    return;
  }
  const int32_t l = sent_len[s];
  if ((l & kLenMask) == 0) return;
  const int64_t k = ks_pos[s];
  ks_start[k] = sent_off[s];
  ks_len[k] = l;
  kscan[k] = tok_pos[s];
}

__global__ void scatter_docs_kernel(const int64_t* doc_sent_off, int64_t n_doc, const int64_t* ks_pos,
                                    const int64_t* kd_pos, int64_t* kd_off) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d > n_doc) return;
  if (d == n_doc) { kd_off[kd_pos[n_doc]] = ks_pos[doc_sent_off[n_doc]]; return; }
  if (kd_pos[d + 1] > kd_pos[d]) kd_off[kd_pos[d]] = ks_pos[doc_sent_off[d]];
}

__global__ void part_offsets_kernel(const int64_t* part_doc_off, int64_t n_part, const int64_t* kd_pos,
                                    int64_t* kp_off, unsigned long long* max_docs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n_part) kp_off[p] = kd_pos[part_doc_off[p]];
  if (p < n_part)  // kept documents of the largest partition (the planner's LDS table choice)
    atomicMax(max_docs, (unsigned long long)(kd_pos[part_doc_off[p + 1]] - kd_pos[part_doc_off[p]]));
}

}  // namespace

// Drop empty sentences and documents: the kept-sentence tables, the partitions' kept-document
// offsets and the dense token buffer.
int compact_inputs(lddl_pairs* P, PlanWork& W, const int64_t* d_sent_off,
                   const int32_t* d_sent_len, const int64_t* d_doc_sent_off, int64_t n_doc,
                   const int64_t* d_part_doc_off) {
  const int64_t n_sent = W.n_sent, n_part = W.n_part;
  hipStream_t st = W.st;
  int rc;
  int64_t *ks_pos, *tok_pos, *kd_pos;
  const int64_t nscr = 2 * scan_scratch_elems(std::max(n_sent, n_doc) + n_part + 1);  // (dual scans)
  // kept-sentence index and token offset of every sentence in one scan
  if ((rc = W.tmp.take(&W.scratch, nscr)) || (rc = W.tmp.take(&ks_pos, n_sent + 1)) ||
      (rc = W.tmp.take(&tok_pos, n_sent + 1)))
    return rc;
  LDDL_HIP(scan_exclusive2(SentCounts{d_sent_len}, n_sent, ks_pos, tok_pos, W.scratch, st));
  if ((rc = W.tmp.take(&kd_pos, n_doc + 1))) return rc;
  LDDL_HIP(scan_exclusive(KeepDoc{ks_pos, d_doc_sent_off}, n_doc, kd_pos, W.scratch, st));
  int64_t h_counts[3];
  LDDL_HIP(hipMemcpyAsync(&h_counts[0], ks_pos + n_sent, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&h_counts[1], kd_pos + n_doc, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&h_counts[2], tok_pos + n_sent, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  P->n_kept_sent = h_counts[0];
  P->n_kept_doc = h_counts[1];
  W.n_kept_tok = h_counts[2];  // (dropped sentences have no tokens)
  unsigned long long* d_max_docs;
  if ((rc = P->mem.take(&P->ks_start, P->n_kept_sent)) || (rc = P->mem.take(&P->ks_len, P->n_kept_sent)) ||
      (rc = P->mem.take(&P->kscan, P->n_kept_sent + 1)) || (rc = P->mem.take(&P->kd_off, P->n_kept_doc + 1)) ||
      (rc = P->mem.take(&P->kp_off, n_part + 1)) || (rc = W.tmp.take(&d_max_docs, 1)))
    return rc;
  hipLaunchKernelGGL(scatter_sentences_kernel, dim3((unsigned)((n_sent + 256) / 256)), dim3(256), 0,
                     st, d_sent_off, d_sent_len, n_sent, ks_pos, tok_pos, P->ks_start, P->ks_len,
                     P->kscan);
  hipLaunchKernelGGL(scatter_docs_kernel, dim3((unsigned)((n_doc + 256) / 256)), dim3(256), 0, st,
                     d_doc_sent_off, n_doc, ks_pos, kd_pos, P->kd_off);
  LDDL_HIP(hipMemsetAsync(d_max_docs, 0, 8, st));
  hipLaunchKernelGGL(part_offsets_kernel, dim3((unsigned)((n_part + 256) / 256)), dim3(256), 0, st,
                     d_part_doc_off, n_part, kd_pos, P->kp_off, d_max_docs);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipMemcpyAsync(&W.max_docs, d_max_docs, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  // dense kept tokens, 8 tokens of padding on both sides: the gather's 4- and 8-token loads may
  // overhang a window
  const int32_t ib = W.c->id_bytes();
  uint8_t* raw;
  if ((rc = P->mem.take(&raw, (W.n_kept_tok + 16) * ib))) return rc;
  P->dense = IdPtr{raw + 8 * ib, ib};
  if (P->n_kept_sent && !dense_in_plan(W))
    launch_densify(P->ks_start, P->ks_len, P->kscan, P->n_kept_sent, W.d_ids, P->dense, st);
  LDDL_HIP(hipGetLastError());
  return 0;
}

}  // namespace lddl
