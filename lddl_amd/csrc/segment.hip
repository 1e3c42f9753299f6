// Punkt sentence segmentation on the GPU: the reference's `nltk.tokenize.sent_tokenize(text)`
// (lddl/dask/bert/pretrain.py:86) followed by `strip()` + dropping empty sentences (87-88).
//
// nltk's PunktSentenceTokenizer (nltk/tokenize/punkt.py 3.6.5, a third-party dependency of the
// reference) finds candidate contexts with `period_context_re`
//     \S* [.?!] (?= NonWord | \s+ (\S+) )
// (finditer), decides each with `text_contains_sentbreak(context)` (word tokenisation +
// first/second-pass annotation with the trained parameters), cuts slices at the accepted
// contexts and moves closing brackets/quotes across the cut (`_realign_boundaries`).
//
// Structure used here (derivation in DESIGN.md §4):
//  * finditer yields at most one match per whitespace-free run: the match starts at the run's
//    first byte and ends after the LAST sentence-ending char of the run whose lookahead holds;
//  * a lookahead holds at q iff text[q+1] is a NonWord char, or whitespace with some
//    non-whitespace later in the document (q+1 < rstrip end);
//  * the strip() applied by the reference makes inter-sentence whitespace irrelevant, and the
//    BERT tokenizer ignores whitespace, so each sentence is emitted as [boundary_k,
//    boundary_{k+1}) with the gaps attached to the left sentence: the sentence offsets feed
//    lddl_tokenize directly (documents are contiguous, so the last sentence of a document ends
//    where the next document starts).
//  * the realignment of a cut only depends on the bytes after it: boundary = next sentence start
//    + length of a run of closing chars that is followed by whitespace, "--" or the end.
//
// Kernel: one wavefront per document streams 64-byte windows (one byte per lane). Lanes flag
// whitespace (ASCII by a bit test, other code points through the two-level class table) and
// lookahead-qualified sentence enders; ballots give each selected ender its run start; the
// selected lanes then evaluate their context sequentially (rare: ~1 per sentence) and the
// accepted cuts are appended in order (ballot prefix) to a per-document slot range.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>

#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "punkt_dev.h"
#include "punkt_state.h"
#include "scan.h"

namespace lddl {
namespace {

constexpr int kSegWaves = 4;
constexpr int kSlab = 4096;     // LDS bytes per classifying wave
constexpr int kCtx = 64;        // context bytes staged per candidate lane
constexpr int kRowW = 17;       // LDS row stride in dwords (68 B: conflict-free byte walks)
constexpr int kEvalBlock = 256;

// K1: one wavefront per document streams it through a 4-KB LDS slab (four 16-B loads per lane
// in flight), 4 bytes per lane per 256-byte window, and appends each whitespace-free run's match
// -- its last lookahead-qualified sentence ender (text[q] in .?! and text[q+1] NonWord, or
// whitespace with non-whitespace later) -- in order to the document's slot range
// cand[(doc_off[d] - doc_off[0]) / 2 + d ..] (a document of L bytes has at most L/2 + 1
// whitespace-free runs, the bound of both candidates and cuts: "?!?!?! x" has five qualified
// enders in one run, so one per run is what keeps writes inside the range).
// 6 waves per SIMD (<= 80 VGPRs): 5.8 ms per 2 GiB vs 6.1 at the compiler's 96 VGPRs / 5 waves
// and 6.3 at 8 waves (64 VGPRs, spills) -- profiles/r01_v14_segment_variants.txt
__global__ void __launch_bounds__(64 * kSegWaves) __attribute__((amdgpu_waves_per_eu(6))) segment_classify_kernel(
    PunktTab t, const uint8_t* __restrict__ x, int64_t n_bytes, const int64_t* __restrict__ doc_off,
    int64_t n_doc, int32_t* __restrict__ cand, int32_t* __restrict__ ccnt, int32_t* __restrict__ rs_rel,
    int32_t* __restrict__ cnt) {
  __shared__ uint4 slab_all[kSegWaves][kSlab / 16];
  const int64_t d = (int64_t)blockIdx.x * kSegWaves + wave_id();
  if (d >= n_doc) return;  // wave-uniform
  const int lane = lane_id();
  uint4* slab = slab_all[threadIdx.x >> 6];
  const int64_t b0 = doc_off[d], b1 = doc_off[d + 1];
  int32_t* out = cand + ((b0 - doc_off[0]) >> 1) + d;
  const Src g(x, slab, 0, 0);  // global only
  // rstrip end: one past the last non-whitespace byte
  int64_t rs = b0;
  for (int64_t we = b1; we > b0; we -= 64) {
    const int64_t i = we - 64 + lane;
    const bool nonsp = i >= b0 && !space_at(t, g, i, b0, b1);
    const uint64_t m = ballot(nonsp);
    if (m) {
      rs = we - 64 + (63 - __builtin_clzll(m)) + 1;
      break;
    }
  }
  const bool aligned = ((uintptr_t)x & 15u) == 0;
  int32_t nc = 0;
  for (int64_t blk = b0; blk < rs;) {
    const int64_t lo = blk & ~(int64_t)15;
    const int64_t hi = std::min<int64_t>(n_bytes, lo + kSlab);
    wave_sync();  // previous slab consumed
    if (aligned && lo + kSlab <= n_bytes) {  // all loads in flight before the LDS writes
      uint4 v[kSlab / 1024];
#pragma unroll
      for (int r = 0; r < kSlab / 1024; ++r)
        v[r] = *reinterpret_cast<const uint4*>(x + lo + 16 * (int64_t)(lane + 64 * r));
#pragma unroll
      for (int r = 0; r < kSlab / 1024; ++r) slab[lane + 64 * r] = v[r];
    } else {  // end of the text buffer / unaligned text: byte loads
      for (int r = lane; r < kSlab / 16; r += 64) {
        const int64_t a = lo + 16 * (int64_t)r;
        uint8_t tmp[16] = {};
        for (int k = 0; k < 16 && a + k < hi; ++k) tmp[k] = x[a + k];
        uint4 v;
        memcpy(&v, tmp, 16);
        slab[r] = v;
      }
    }
    wave_sync();
    const Src src(x, slab, lo, hi);
    const int64_t bend = std::min<int64_t>(rs, hi);
    const uint32_t* slab32 = reinterpret_cast<const uint32_t*>(slab);
    // 256-byte windows, 4 bytes per lane (one LDS dword); a SWAR test skips words without
    // '.', '?' or '!' (bytes before b0 -- first slab only -- are masked)
    for (int64_t base = lo; base < bend; base += 256) {
      const int64_t i0 = base + 4 * lane;
      const uint32_t w = slab32[(i0 - lo) >> 2];
      const uint32_t x1 = w ^ 0x2E2E2E2Eu, x2 = w ^ 0x3F3F3F3Fu, x3 = w ^ 0x21212121u;
      const uint32_t maybe = ((x1 - 0x01010101u) & ~x1) | ((x2 - 0x01010101u) & ~x2) |
                             ((x3 - 0x01010101u) & ~x3);
      uint32_t qb = 0, nwb = 0;
      if (maybe & 0x80808080u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t pos = i0 + k;
          const uint32_t c = (w >> (8 * k)) & 255u;
          if (pos < b0 || pos >= bend || !sent_end(c) || pos + 1 >= rs) continue;
          const uint32_t cn = k < 3 ? (w >> (8 * k + 8)) & 255u : src[pos + 1];
          if (non_word(cn))
            nwb |= 1u << k;
          else if (cn < 0x80 ? ascii_space(cn) : space_at(t, src, pos + 1, b0, b1))
            qb |= 1u << k;
        }
      }
      // a NonWord lookahead is a match only if it is the run's LAST qualified ender (finditer):
      // scan the rest of the run (rare; kept out of the unrolled loop above so its registers do
      // not cost occupancy). This also keeps the candidates within the per-document slot range.
      for (uint32_t m = nwb; m; m &= m - 1) {
        const int64_t pos = i0 + __builtin_ctz(m);
        bool last = true;
        for (int64_t q = pos + 1; q < rs && last; ++q) {
          if (space_at(t, src, q, b0, b1)) break;
          if (sent_end(src[q]) && q + 1 < rs && (non_word(src[q + 1]) || space_at(t, src, q + 1, b0, b1)))
            last = false;
        }
        if (last) qb |= m & (~m + 1);
      }
      if (ballot(qb != 0)) {  // append this window's enders in position order
        const int n = __builtin_popcount(qb);
        const int incl = wave_incl_scan(n);
        int slot = nc + incl - n;
        for (uint32_t m = qb; m; m &= m - 1) out[slot++] = (int32_t)(i0 + __builtin_ctz(m) - b0);
        nc += __shfl(incl, 63, 64);
      }
    }
    blk = bend;
  }
  if (lane == 0) {
    ccnt[d] = nc;
    rs_rel[d] = (int32_t)(rs - b0);
    cnt[d] = 1;
  }
}

struct CntAt {
  const int32_t* cnt;
  __device__ int64_t operator()(int64_t i) const { return cnt[i]; }
};

// K1b: candidates into one flat list (position, document), in document order
__global__ void segment_flatten_kernel(const int64_t* __restrict__ doc_off, int64_t n_doc,
                                       const int32_t* __restrict__ cand, const int64_t* __restrict__ coff,
                                       int64_t* __restrict__ fq, int32_t* __restrict__ fdoc) {
  const int64_t d = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_id();
  if (d >= n_doc) return;
  const int64_t b0 = doc_off[d];
  const int32_t* in = cand + ((b0 - doc_off[0]) >> 1) + d;
  const int64_t o = coff[d], n = coff[d + 1] - o;
  for (int64_t k = lane_id(); k < n; k += 64) {
    fq[o + k] = b0 + in[k];
    fdoc[o + k] = (int32_t)d;
  }
}

// K2: one lane per candidate. The lane stages 64 bytes around its ender in a private LDS row
// (four 16-B loads issued together), then walks the context from LDS (Src falls back to global
// memory outside the row). fbound = realigned cut position, or -1; cnt[d] counts the cuts.
template <bool kParams>
__global__ void __launch_bounds__(kEvalBlock) segment_eval_kernel(
    PunktTab t, const uint8_t* __restrict__ x, int64_t n_bytes, const int64_t* __restrict__ doc_off,
    const int32_t* __restrict__ rs_rel, const int64_t* __restrict__ fq, const int32_t* __restrict__ fdoc,
    int64_t n_cand, int64_t* __restrict__ fbound, int32_t* __restrict__ cnt) {
  __shared__ uint32_t rows[kEvalBlock * kRowW];
  if (!kParams) t.n_rec = 0;
  const int64_t c = (int64_t)blockIdx.x * kEvalBlock + threadIdx.x;
  if (c >= n_cand) return;
  uint32_t* row = rows + threadIdx.x * kRowW;
  const int64_t q = fq[c];
  const int32_t d = fdoc[c];
  const int64_t b0 = doc_off[d], b1 = doc_off[d + 1], rs = b0 + rs_rel[d];
  const int64_t w0 = std::max<int64_t>(0, (q - 24) & ~(int64_t)15);
  const int64_t w1 = std::min<int64_t>(n_bytes, w0 + kCtx);
  uint4 v[kCtx / 16];
  const bool aligned = ((uintptr_t)x & 15u) == 0;
#pragma unroll
  for (int k = 0; k < kCtx / 16; ++k) {
    const int64_t a = w0 + 16 * k;
    v[k] = make_uint4(0, 0, 0, 0);
    if (a + 16 <= w1 && aligned) {
      v[k] = *reinterpret_cast<const uint4*>(x + a);
    } else if (a < w1) {
      uint8_t tmp[16] = {};
      for (int j = 0; j < 16 && a + j < w1; ++j) tmp[j] = x[a + j];
      memcpy(&v[k], tmp, 16);
    }
  }
#pragma unroll
  for (int k = 0; k < kCtx / 16; ++k) {
    row[4 * k] = v[k].x;
    row[4 * k + 1] = v[k].y;
    row[4 * k + 2] = v[k].z;
    row[4 * k + 3] = v[k].w;
  }
  const Src src(x, row, w0, w1);
  int64_t bound = -1;
  const bool cut = eval_candidate<kParams>(t, src, q, b0, b1, rs, &bound);
  fbound[c] = cut ? bound : -1;
  if (cut) atomicAdd(&cnt[d], 1);
}

// sent_off[doc_sent_off[d] + k]: document start, then its cuts in order; sent_off[n_sent] = end
__global__ void segment_fill_kernel(const int64_t* __restrict__ doc_off, int64_t n_doc,
                                    const int64_t* __restrict__ coff, const int64_t* __restrict__ fbound,
                                    const int64_t* __restrict__ dso, int64_t* __restrict__ sent_off) {
  const int64_t d = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_id();
  if (d >= n_doc) return;
  const int lane = lane_id();
  const int64_t o = dso[d];
  if (lane == 0) sent_off[o] = doc_off[d];
  int64_t k = o + 1;
  for (int64_t base = coff[d], e = coff[d + 1]; base < e; base += 64) {
    const int64_t j = base + lane;
    const int64_t bnd = j < e ? fbound[j] : -1;
    const uint64_t m = ballot(bnd >= 0);
    if (bnd >= 0) sent_off[k + popc_below(m)] = bnd;
    k += __builtin_popcountll(m);
  }
  if (d == n_doc - 1 && lane == 0) sent_off[dso[n_doc]] = doc_off[n_doc];
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_segment_count(lddl_ctx* c, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                  const int64_t* d_doc_off, int64_t n_doc, int64_t* n_sent) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  lddl_punkt_state* ps = c->punkt;
  if (!ps || !ps->tab.cls.l1) LDDL_FAIL(-1, "Punkt parameters not set (lddl_punkt_set_params)");
  if (n_doc < 0 || n_bytes < 0 || !n_sent) LDDL_FAIL(-1, "bad sizes");
  if (ps->pending) LDDL_FAIL(-1, "a segmentation is pending: call lddl_segment_fill first");
  hipStream_t st = as_stream(stream);
  // local until the count is complete: an error return gives the blocks back
  auto S = std::make_unique<PendingSeg>(&c->arena, st);
  const int64_t nd = n_doc + 1;
  int rc;
  if ((rc = S->mem.take(&S->cand, n_bytes / 2 + n_doc + 2)) || (rc = S->mem.take(&S->ccnt, nd)) ||
      (rc = S->mem.take(&S->rs_rel, nd)) || (rc = S->mem.take(&S->cnt, nd)) ||
      (rc = S->mem.take(&S->coff, nd)) || (rc = S->mem.take(&S->dso, nd)) ||
      (rc = S->mem.take(&S->scratch, scan_scratch_elems(n_doc))))
    return rc;
  const PunktTab& t = ps->tab;
  const int64_t dgrid = std::max<int64_t>(1, (n_doc + kSegWaves - 1) / kSegWaves);
  if (n_doc > 0) {
    hipLaunchKernelGGL(segment_classify_kernel, dim3((unsigned)dgrid), dim3(64 * kSegWaves), 0, st, t, d_text,
                       n_bytes, d_doc_off, n_doc, S->cand, S->ccnt, S->rs_rel, S->cnt);
    LDDL_HIP(hipGetLastError());
  }
  LDDL_HIP(scan_exclusive(CntAt{S->ccnt}, n_doc, S->coff, S->scratch, st));
  int64_t n_cand = 0;
  LDDL_HIP(hipMemcpyAsync(&n_cand, S->coff + n_doc, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  if ((rc = S->mem.take(&S->fq, n_cand)) || (rc = S->mem.take(&S->fdoc, n_cand)) ||
      (rc = S->mem.take(&S->fbound, n_cand)))
    return rc;
  if (n_cand > 0) {
    hipLaunchKernelGGL(segment_flatten_kernel, dim3((unsigned)dgrid), dim3(64 * kSegWaves), 0, st, d_doc_off,
                       n_doc, (const int32_t*)S->cand, S->coff, S->fq, S->fdoc);
    const int64_t egrid = (n_cand + kEvalBlock - 1) / kEvalBlock;
    auto eval = t.n_rec ? segment_eval_kernel<true> : segment_eval_kernel<false>;  // (trained parameters?)
    hipLaunchKernelGGL(eval, dim3((unsigned)egrid), dim3(kEvalBlock), 0, st, t, d_text, n_bytes, d_doc_off,
                       (const int32_t*)S->rs_rel, (const int64_t*)S->fq, (const int32_t*)S->fdoc, n_cand,
                       S->fbound, S->cnt);
    LDDL_HIP(hipGetLastError());
  }
  LDDL_HIP(scan_exclusive(CntAt{S->cnt}, n_doc, S->dso, S->scratch, st));
  LDDL_HIP(hipMemcpyAsync(n_sent, S->dso + n_doc, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  S->doc_off = d_doc_off;
  S->n_doc = n_doc;
  ps->pending = std::move(S);
  return 0;
}

extern "C" int lddl_segment_fill(lddl_ctx* c, void* stream, int64_t* d_sent_off, int64_t* d_doc_sent_off) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  lddl_punkt_state* ps = c->punkt;
  if (!ps || !ps->pending) LDDL_FAIL(-1, "no pending segmentation (lddl_segment_count)");
  if (!d_sent_off != !d_doc_sent_off) LDDL_FAIL(-1, "lddl_segment_fill: null output");
  hipStream_t st = as_stream(stream);
  // the call ends the pending segmentation, whatever it returns (both outputs null: cancel)
  std::unique_ptr<PendingSeg> S = std::move(ps->pending);
  int rc = 0;
  if (d_sent_off) {
    const int64_t n_doc = S->n_doc;
    if (n_doc > 0) {
      const int64_t grid = (n_doc + 3) / 4;
      hipLaunchKernelGGL(segment_fill_kernel, dim3((unsigned)grid), dim3(256), 0, st, S->doc_off, n_doc,
                         (const int64_t*)S->coff, (const int64_t*)S->fbound, (const int64_t*)S->dso,
                         d_sent_off);
    } else {
      if (hipMemsetAsync(d_sent_off, 0, sizeof(int64_t), st) != hipSuccess) rc = -100;
    }
    if (hipMemcpyAsync(d_doc_sent_off, S->dso, sizeof(int64_t) * (size_t)(n_doc + 1), hipMemcpyDeviceToDevice,
                       st) != hipSuccess)
      rc = -100;
    if (hipGetLastError() != hipSuccess) rc = -100;
  }
  S->mem.release(st);
  if (rc) LDDL_FAIL(rc, "lddl_segment_fill: HIP launch/copy failed");
  return 0;
}
