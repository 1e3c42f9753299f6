// The GPT stream's plan (include/lddl_amd.h states the semantics): where every
// document of a round lies in the endless stream doc, eos, doc, eos, ... that the rows are cut
// from.
//
//   tokens   one scan_exclusive over the masked sentence lengths -> sent_tok_off[n_sent + 1]
//   places   one scan_exclusive over the places: its functor reads doc_order[j], takes t from
//            two entries of the first scan and makes the document's Philox draw for the three
//            sentinels of a transformed document (stream_doc) -> doc_off = Q[n_doc + 1]
//   rows     one thread: n_rows = max(0, (Q[n_doc] - 1) / L) and the total
//
// No host wait, no atomics, no record of the draws (the rows draw them again); the scans'
// scratch comes from a DevArena that this unit owns per device.
#include <map>
#include <mutex>

#include "arena.h"
#include "common.h"
#include "ctx.h"
#include "scan.h"
#include "stream_dev.h"

namespace lddl {
namespace {

struct SentTokens {
  const int32_t* sent_len;
  __device__ int64_t operator()(int64_t s) const { return sent_len[s] & kLenMask; }
};

__global__ void stream_count_kernel(const int64_t* Q, int64_t n_doc, int32_t L, int64_t* out) {
  const int64_t total = Q[n_doc], n = (total - 1) / L;
  out[0] = total > 0 && n > 0 ? n : 0;
  out[1] = total;
}

std::mutex g_mu;
std::map<int, DevArena*> g_arenas;
DevArena* plan_arena() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> g(g_mu);
  DevArena*& a = g_arenas[dev];
  if (!a) a = new DevArena;
  return a;
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_stream_plan(void* stream, const int32_t* d_sent_len, int64_t n_sent,
                                const int64_t* d_doc_sent_off, int64_t n_doc,
                                const int64_t* d_doc_order, int32_t seq_len, int32_t fim_q,
                                int32_t spm_q, uint64_t seed, uint64_t counter,
                                int64_t* d_sent_tok_off, int64_t* d_doc_off, int64_t* d_n_rows) {
  if (seq_len < 1 || seq_len > (1 << 20)) LDDL_FAIL(-1, "seq_len %d is outside [1, 2^20]", seq_len);
  if (fim_q < 0 || fim_q > 65536 || spm_q < 0 || spm_q > 65536)
    LDDL_FAIL(-1, "fim_q %d or spm_q %d is outside [0, 65536]", fim_q, spm_q);
  if (n_sent < 0 || n_doc < 0) LDDL_FAIL(-1, "negative size");
  if (!d_sent_tok_off || !d_doc_off || !d_n_rows) LDDL_FAIL(-1, "null output");
  if (n_sent > 0 && !d_sent_len) LDDL_FAIL(-1, "null sent_len");
  if (n_doc > 0 && !d_doc_sent_off) LDDL_FAIL(-1, "null doc_sent_off");
  hipStream_t st = as_stream(stream);
  DevArena* arena = plan_arena();
  if (!arena) LDDL_FAIL(-100, "no current device");
  ArenaScope tmp(arena, st);
  int64_t* scan_tmp;
  if (tmp.take(&scan_tmp, scan_scratch_elems(n_sent > n_doc ? n_sent : n_doc))) return -100;
  LDDL_HIP(scan_exclusive(SentTokens{d_sent_len}, n_sent, d_sent_tok_off, scan_tmp, st));
  const StreamSrc S{d_doc_sent_off, d_doc_order, d_sent_tok_off, n_sent, n_doc,
                    (uint32_t)fim_q, (uint32_t)spm_q, seed, counter};
  LDDL_HIP(scan_exclusive(StreamCost{S}, n_doc, d_doc_off, scan_tmp, st));
  hipLaunchKernelGGL(stream_count_kernel, dim3(1), dim3(1), 0, st, d_doc_off, n_doc, seq_len,
                     d_n_rows);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_stream_release(void) {
  std::lock_guard<std::mutex> g(g_mu);
  for (auto& kv : g_arenas) kv.second->trim();
  return 0;
}
