// The scan's one-workgroup kernels over the block sums (scan.h declares them; every unit that
// scans launches these) and the C entry point of the scan over a plain int64 array.
#include "scan.h"

#include "common.h"
#include "ctx.h"
#include "lddl_amd.h"

namespace lddl {

__device__ void scan_sums_block(int64_t* sums, int64_t nb) {
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kScanThreads) {
    const int64_t i = b0 + threadIdx.x;
    const int64_t v = i < nb ? sums[i] : 0;
    int64_t tot;
    const int64_t ex = block_excl_scan(v, &tot);
    if (i < nb) sums[i] = carry + ex;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ void __launch_bounds__(kScanThreads) scan_sums_kernel(int64_t* sums, int64_t nb) {
  scan_sums_block(sums, nb);
}

__global__ void __launch_bounds__(kScanThreads) scan_sums2_kernel(int64_t* sa, int64_t* sb, int64_t nb) {
  scan_sums_block(blockIdx.x ? sb : sa, nb);
}

}  // namespace lddl

using namespace lddl;

extern "C" int lddl_scan_i64(lddl_ctx* c, void* stream, const int64_t* d_in, int64_t n,
                             int64_t* d_out) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (n < 0) LDDL_FAIL(-1, "bad size");
  hipStream_t st = as_stream(stream);
  ArenaTmp scratch(&c->arena, st);
  LDDL_HIP(scratch.take(sizeof(int64_t) * scan_scratch_elems(n)));
  struct In {
    const int64_t* v;
    __device__ int64_t operator()(int64_t i) const { return v[i]; }
  };
  LDDL_HIP(scan_exclusive(In{d_in}, n, d_out, scratch.as<int64_t>(), st));
  return 0;
}
