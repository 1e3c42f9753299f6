// Pair stage, random.shuffle(partition_pairs) of the replay plan (lddl/dask/bert/pretrain.py:401):
// the planner's recorded draws resolved into each partition's output order and the pair maps.
#include "pairs_plan.h"

namespace lddl {
namespace {

// The final per-partition Fisher-Yates swaps (draws from plan_replay_kernel) for partitions too
// large for shuffle_sort_kernel's LDS tables (more than min_np pairs): one lane swaps in global
// memory.

__global__ void __launch_bounds__(64) apply_shuffle_kernel(const int64_t* kd_off, const int64_t* kp_off,
                                                          int32_t dup, const int64_t* part_npairs,
                                                          const int32_t* jseq, int32_t* order,
                                                          int64_t min_np) {
  const int p = blockIdx.x;
  const int64_t base = (int64_t)dup * kd_off[kp_off[p]];
  const int64_t np = part_npairs[p];
  if (np <= min_np) return;  // (shuffle_sort_kernel's)
  const int32_t* js = jseq + base;
  int32_t* ord = order + base;
  for (int64_t k = threadIdx.x; k < np; k += 64) ord[k] = (int32_t)k;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int64_t i = np - 1; i > 0; --i) {
      const int32_t j = js[i];
      const int32_t t = ord[i];
      ord[i] = ord[j];
      ord[j] = t;
    }
  }
}

// The same permutation with no sequential chain at all (one workgroup of 1024 per partition of at
// most `cap` pairs; larger ones go to apply_shuffle_kernel). The backward Fisher-Yates
// x[i] <-> x[j_i], i = n-1 .. 1, on x = identity leaves, with succ(i) = the next step k > i that
// drew the same j (j_k = j_i) and first(v) = the first step that drew v:
//   x[i] = succ(i) ? R(succ(i)) : j_i  (i >= 1),   x[0] = first(0) ? R(first(0)) : 0,
// where R(k) follows f(k) = (j_k == k ? succ(k) : first(k)) to the end of its chain (the value
// step k moved out of position k is the one the last earlier-executed step wrote there, and so
// on). succ and first come from a bucket sort of the steps by their draw (LDS counters, a block
// scan, a scatter, then each bucket - a few steps on average - sorted by step), R from pointer
// jumping, everything over 1024 threads. LDS: three 16-bit arrays of n (the draws are read from
// global memory once, coalesced, into the one that later holds f and R).
__device__ inline uint32_t lds_add16(uint32_t* words, uint32_t v) {  // 16-bit counters, packed
  const uint32_t sh = 16u * (v & 1u);
  return (atomicAdd(&words[v >> 1], 1u << sh) >> sh) & 0xFFFFu;
}

constexpr int kShufThreads = 1024;  // one block per CU (its LDS): 16 waves hide the latencies
__global__ void __launch_bounds__(kShufThreads) shuffle_sort_kernel(const int64_t* kd_off, const int64_t* kp_off,
                                                          int32_t dup, const int64_t* part_npairs,
                                                          const int32_t* __restrict__ jseq,
                                                          int32_t* __restrict__ order, int32_t cap,
                                                          PairMaps M) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ss_smem[];
  const int p = blockIdx.x;
  const int32_t n = (int32_t)part_npairs[p];
  if (n > cap) return;  // (apply_shuffle_kernel's)
  const int32_t capw = (cap + 2) & ~1;
  uint32_t* cntw = reinterpret_cast<uint32_t*>(ss_smem);        // bucket counters -> ends
  uint16_t* cnt = reinterpret_cast<uint16_t*>(ss_smem);
  uint16_t* srt = reinterpret_cast<uint16_t*>(ss_smem) + capw;  // steps by bucket
  uint16_t* r = srt + capw;                                     // j, then f, then R
  const int64_t base = (int64_t)dup * kd_off[kp_off[p]];
  const int32_t* __restrict__ js = jseq + base;
  // succ(i) (or ~j_i when step i is the last to draw j_i), then the permutation
  int32_t* __restrict__ ord = order + base;
  const int tid = threadIdx.x;
  for (int32_t w = tid; w < capw / 2; w += kShufThreads) cntw[w] = 0u;
  for (int32_t i = tid; i < n; i += kShufThreads) r[i] = (uint16_t)js[i];
  __syncthreads();
  for (int32_t i = 1 + tid; i < n; i += kShufThreads) (void)lds_add16(cntw, r[i]);
  __syncthreads();
  {  // exclusive scan of the counts: a run per thread, then the runs' sums
    __shared__ int32_t s_w[kShufThreads / 64];
    const int32_t per = (n + kShufThreads - 1) / kShufThreads;
    const int32_t x0 = tid * per, x1 = min(x0 + per, n);
    int32_t run = 0;
    for (int32_t x = x0; x < x1; ++x) run += cnt[x];
    const int32_t inc = wave_incl_scan(run);
    if ((tid & 63) == 63) s_w[tid >> 6] = inc;
    __syncthreads();
    int32_t off = inc - run;
    for (int w = 0; w < (tid >> 6); ++w) off += s_w[w];
    for (int32_t x = x0; x < x1; ++x) {
      const int32_t c = cnt[x];
      cnt[x] = (uint16_t)off;
      off += c;
    }
  }
  __syncthreads();
  for (int32_t i = 1 + tid; i < n; i += kShufThreads) srt[lds_add16(cntw, r[i])] = (uint16_t)i;
  __syncthreads();  // cnt[v] = the end of bucket v now
  // each bucket sorted by step (insertion sort: a few entries), succ along it
  for (int32_t v = tid; v < n; v += kShufThreads) {
    const int32_t lo = v ? cnt[v - 1] : 0, hi = cnt[v];
    for (int32_t m = lo + 1; m < hi; ++m) {
      const uint16_t e = srt[m];
      int32_t y = m - 1;
      while (y >= lo && srt[y] > e) {
        srt[y + 1] = srt[y];
        --y;
      }
      srt[y + 1] = e;
    }
    for (int32_t m = lo; m < hi; ++m) ord[srt[m]] = m + 1 < hi ? (int32_t)srt[m + 1] : ~v;
  }
  __syncthreads();
  // f(k) = j_k == k ? succ(k) : first(k); R(k) = k at a chain's end (each thread reads the
  // draws it overwrites)
  for (int32_t k = tid; k < n; k += kShufThreads) {
    int32_t f = -1;
    if (k > 0) {
      if (r[k] == k) {
        f = ord[k];
      } else {
        const int32_t lo = cnt[k - 1], hi = cnt[k];
        f = lo < hi ? (int32_t)srt[lo] : -1;
      }
    }
    r[k] = (uint16_t)(f < 0 ? k : f);
  }
  __syncthreads();
  for (;;) {  // pointer jumping: R(k) = R(R(k)) until every chain is collapsed
    int changed = 0;
    for (int32_t k = tid; k < n; k += kShufThreads) {
      const uint16_t a = r[k], b = r[a];
      if (b != a) {
        r[k] = b;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  const int32_t first0 = n > 1 && cnt[0] > 0 ? (int32_t)srt[0] : -1;
  const int64_t q0 = M.part_base ? M.part_base[p] : 0;
  for (int32_t k = tid; k < n; k += kShufThreads) {
    const int32_t sc = k == 0 ? first0 : ord[k];
    const int32_t v = sc >= 0 ? (int32_t)r[sc] : (k == 0 ? 0 : ~sc);
    ord[k] = v;
    if (M.src) M.src[q0 + k] = base + v;
    if (M.slots) M.slots[q0 + k] = base + k;
    if (M.dstq) M.dstq[q0 + v] = q0 + k;
  }
}

// src[q]: the planner slot of output pair q (partition shuffle applied); slots[q]: the q-th
// slot in planner order (every partition's slots base .. base + np - 1), so the per-slot passes
// read the slot-indexed arrays front to back instead of in shuffled order.
// (any output may be null)
// dstq[i]: the output position of the i-th pair in planner order (the inverse of src), for the
// mask replay that also writes each pair's gather record.
__global__ void map_pairs_kernel(const int64_t* kd_off, const int64_t* kp_off, int32_t dup,
                                 const int64_t* part_pair_base, const int32_t* order, int64_t* src,
                                 int64_t* slots, int64_t* dstq) {
  const int p = blockIdx.x;
  const int64_t base = (int64_t)dup * kd_off[kp_off[p]];
  const int64_t q0 = part_pair_base[p], n = part_pair_base[p + 1] - q0;
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
    if (src) src[q0 + k] = base + order[base + k];
    if (slots) slots[q0 + k] = base + k;
    if (dstq) dstq[q0 + order[base + k]] = q0 + k;
  }
}

}  // namespace

// random.shuffle(partition_pairs) of one range, alone on the stream (its blocks need 16 waves
// and ~90 KB of LDS per CU: beside fy_resolve's small blocks on a second stream they waited for
// CUs to drain, 10.3 ms against ~2 alone); its last pass writes the pair maps (see PairMaps): with
// masking the planner-order slots and their output positions (the mask replay writes each
// pair's gather record there), else the output order. rel_base[i]: the first pair of the
// range's partition i, counted from the range's first pair.
int shuffle_partitions(lddl_pairs* P, PlanWork& W, const PairRange& r, const int64_t* rel_base) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = r.p1 - r.p0;
  hipStream_t st = W.st;
  int rc;
  PairMaps& M = W.rt.M;
  M = PairMaps{rel_base, nullptr, nullptr, nullptr};
  if (prm->masking) {
    if ((rc = W.tmp.take(&M.slots, r.n_pairs)) || (rc = W.tmp.take(&M.dstq, r.n_pairs))) return rc;
  } else {
    if ((rc = P->mem.take(&P->src, r.n_pairs))) return rc;
    M.src = P->src;
  }
  if (n_part) {
    const int64_t cap = W.max_np;
    const int64_t* kp_off = P->kp_off + r.p0;  // (the kernels index partitions by workgroup)
    const int64_t* part_npairs = W.part_npairs + r.p0;
    // dynamic-LDS budget of the swap kernel: what the device grants a block (160 KiB on
    // gfx950), minus headroom for the kernel's static LDS
    const size_t kLdsBudget = std::min<size_t>(150 * 1024, W.c->lds_per_block > 10 * 1024
                                                               ? W.c->lds_per_block - 10 * 1024 : 0);
    const bool force_global = W.knobs.shuffle_global;  // LDDL_SHUFFLE_GLOBAL, tests: the large-partition path
    // partitions of <= cap_lds pairs: the parallel bucket-sort resolve (three 16-bit LDS tables);
    // larger ones: one lane swapping in global memory
    const int64_t cap_lds = force_global ? 0 : std::min<int64_t>({cap, 65534, (int64_t)(kLdsBudget / 6) - 2});
    if (cap_lds > 0)
      hipLaunchKernelGGL(shuffle_sort_kernel, dim3((unsigned)n_part), dim3(kShufThreads),
                         (size_t)6 * (size_t)((cap_lds + 2) & ~1), st, P->kd_off, kp_off,
                         prm->dup, part_npairs, W.jseq, P->order, (int32_t)cap_lds, M);
    if (cap > cap_lds) {  // partitions beyond the LDS tables: swaps in global memory, then the maps
      hipLaunchKernelGGL(apply_shuffle_kernel, dim3((unsigned)n_part), dim3(64), 0, st, P->kd_off,
                         kp_off, prm->dup, part_npairs, W.jseq, P->order, cap_lds);
      hipLaunchKernelGGL(map_pairs_kernel, dim3((unsigned)n_part), dim3(256), 0, st, P->kd_off,
                         kp_off, prm->dup, M.part_base, (const int32_t*)P->order, M.src, M.slots,
                         M.dstq);
    }
  }
  LDDL_HIP(hipGetLastError());
  return 0;
}

}  // namespace lddl
