// Sample table -> output layout on the GPU, first step: sequence-length binning, per partition
// and of one large segment. The rendering of the parquet columns is output_render.hip.
//
// Reference:
//   _to_dataframe_binned           lddl/dask/bert/binning.py:63-93   -> bin_partitions_kernel
//     bin_id = min((num_tokens - 1) // bin_size, nbins - 1); rows of a partition regrouped by bin,
//     stable within a bin (pd.concat of per-bin frames in bin order).
//
// bin_partitions_kernel: one workgroup per partition. Pass 1 counts rows per bin in LDS; an LDS
// scan turns counts into bin bases; pass 2 walks the partition in order 64 rows at a time and
// ranks each row among earlier rows of the same bin: running per-bin counter (LDS) + the lanes
// below it with the same bin, found with bit-sliced ballots (one ballot per bit of the bin id).
// Only wave 0 runs pass 2, so the per-bin counters need no atomics and order is preserved.
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "scan.h"

namespace lddl {
namespace {

constexpr int kBinThreads = 256;
constexpr int kMaxBinsLds = 8192;

__device__ inline int32_t bin_of(int32_t nt, int32_t bin_size, int32_t nbins) {
  const int32_t b = (nt - 1) / bin_size;  // num_tokens >= 5 (>= 1 token in A and in B)
  return b > nbins - 1 ? nbins - 1 : b;
}

// num_tokens of row r: an int32 column, or (tok_off given) the pair's token count + 3
struct NumTok {
  const int32_t* nt;
  const int64_t* tok_off;
  __device__ int32_t operator[](int64_t r) const {
    return nt ? nt[r] : (int32_t)(tok_off[r + 1] - tok_off[r] + 3);
  }
};

__global__ void __launch_bounds__(kBinThreads) bin_partitions_kernel(
    NumTok num_tokens, const int64_t* __restrict__ part_off, int32_t bin_size,
    int32_t nbins, int32_t nbits, int64_t* __restrict__ perm, int64_t* __restrict__ bin_id,
    int64_t* __restrict__ counts) {
  __shared__ int64_t s_cnt[kMaxBinsLds];
  __shared__ int64_t s_tot[kBinThreads / 64];
  const int64_t p = blockIdx.x;
  const int64_t r0 = part_off[p], r1 = part_off[p + 1];
  for (int b = threadIdx.x; b < nbins; b += kBinThreads) s_cnt[b] = 0;
  __syncthreads();
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kBinThreads)
    atomicAdd(reinterpret_cast<unsigned long long*>(&s_cnt[bin_of(num_tokens[r], bin_size, nbins)]),
              1ull);
  __syncthreads();
  // counts out, then exclusive scan of s_cnt in place (bins in chunks of kBinThreads)
  for (int b = threadIdx.x; b < nbins; b += kBinThreads) counts[p * nbins + b] = s_cnt[b];
  int64_t carry = 0;
  for (int b0 = 0; b0 < nbins; b0 += kBinThreads) {
    const int b = b0 + threadIdx.x;
    const int64_t v = b < nbins ? s_cnt[b] : 0;
    const int64_t incl = wave_incl_scan(v);
    if (lane_id() == 63) s_tot[threadIdx.x >> 6] = incl;
    __syncthreads();
    int64_t off = carry;
    int64_t tot = 0;
    for (int w = 0; w < kBinThreads / 64; ++w) {
      if (w < (int)(threadIdx.x >> 6)) off += s_tot[w];
      tot += s_tot[w];
    }
    __syncthreads();
    if (b < nbins) s_cnt[b] = off + incl - v;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1;
  for (int64_t c0 = r0; c0 < r1; c0 += 64) {
    const int64_t r = c0 + lane;
    const bool in = r < r1;
    const int32_t b = in ? bin_of(num_tokens[r], bin_size, nbins) : -1;
    uint64_t match = ballot(in);
    for (int k = 0; k < nbits; ++k) {
      const uint64_t bk = ballot(in && ((b >> k) & 1));
      match &= ((b >> k) & 1) ? bk : ~bk;
    }
    const int rank = (int)popc_below(match);
    int64_t base = 0;
    if (in) base = s_cnt[b];
    __builtin_amdgcn_wave_barrier();
    if (in) {
      const int64_t dst = r0 + base + rank;
      perm[dst] = r;
      bin_id[dst] = b;
      if ((match & below) == 0) s_cnt[b] = base + __popcll(match);  // group leader advances
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}


// ---- stable sort by bin of one large segment: tiles of kBinTile rows, one wavefront each ----
constexpr int kBinTile = 2048;


__global__ void __launch_bounds__(64) bin_tile_hist_kernel(NumTok num_tokens,
                                                           int64_t n, int32_t bin_size,
                                                           int32_t nbins, int64_t n_tiles,
                                                           int64_t* __restrict__ tile_counts) {
  __shared__ int32_t s_cnt[kMaxBinsLds];
  const int64_t tile = blockIdx.x;
  for (int b = threadIdx.x; b < nbins; b += 64) s_cnt[b] = 0;
  __syncthreads();
  const int64_t r0 = tile * kBinTile, r1 = min(n, r0 + kBinTile);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 64)
    atomicAdd(&s_cnt[bin_of(num_tokens[r], bin_size, nbins)], 1);
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += 64) tile_counts[(int64_t)b * n_tiles + tile] = s_cnt[b];
}

__global__ void __launch_bounds__(64) bin_tile_scatter_kernel(
    NumTok num_tokens, int64_t n, int32_t bin_size, int32_t nbins,
    int32_t nbits, int64_t n_tiles, const int64_t* __restrict__ tile_base,
    int64_t* __restrict__ perm, int64_t* __restrict__ bin_id) {
  __shared__ int64_t s_run[kMaxBinsLds];
  const int64_t tile = blockIdx.x;
  for (int b = threadIdx.x; b < nbins; b += 64) s_run[b] = tile_base[(int64_t)b * n_tiles + tile];
  __syncthreads();
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1;
  const int64_t r0 = tile * kBinTile, r1 = min(n, r0 + kBinTile);
  for (int64_t c0 = r0; c0 < r1; c0 += 64) {
    const int64_t r = c0 + lane;
    const bool in = r < r1;
    const int32_t b = in ? bin_of(num_tokens[r], bin_size, nbins) : -1;
    uint64_t match = ballot(in);
    for (int k = 0; k < nbits; ++k) {
      const uint64_t bk = ballot(in && ((b >> k) & 1));
      match &= ((b >> k) & 1) ? bk : ~bk;
    }
    int64_t base = 0;
    if (in) base = s_run[b];
    __builtin_amdgcn_wave_barrier();
    if (in) {
      const int64_t dst = base + (int)popc_below(match);
      perm[dst] = r;
      if (bin_id) bin_id[dst] = b;
      if ((match & below) == 0) s_run[b] = base + __popcll(match);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// bin totals = column sums of the tile counts (bin b's tiles are contiguous after the scan)
__global__ void bin_totals_kernel(const int64_t* __restrict__ tile_base, int64_t n_tiles,
                                  int32_t nbins, int64_t* __restrict__ counts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nbins) counts[b] = tile_base[(int64_t)(b + 1) * n_tiles] - tile_base[(int64_t)b * n_tiles];
}

}  // namespace
}  // namespace lddl

using namespace lddl;

extern "C" int lddl_bin_partitions(lddl_ctx* c, void* stream, const int32_t* d_num_tokens,
                                   const int64_t* d_tok_off, int64_t n_rows,
                                   const int64_t* d_part_off, int64_t n_part, int32_t bin_size,
                                   int32_t nbins, int64_t* d_perm, int64_t* d_bin_id,
                                   int64_t* d_counts) {
  (void)c;
  if (bin_size < 1 || nbins < 1) LDDL_FAIL(-1, "bin_size and nbins must be >= 1");
  if (nbins > kMaxBinsLds) LDDL_FAIL(-1, "nbins %d > %d unsupported", nbins, kMaxBinsLds);
  if (n_part < 0 || n_rows < 0) LDDL_FAIL(-1, "bad sizes");
  if (!d_num_tokens && !d_tok_off && n_rows) LDDL_FAIL(-1, "need num_tokens or tok_off");
  if (n_part == 0) return 0;
  int nbits = 0;
  while ((1 << nbits) < nbins) ++nbits;
  hipLaunchKernelGGL(bin_partitions_kernel, dim3((unsigned)n_part), dim3(kBinThreads), 0,
                     as_stream(stream), NumTok{d_num_tokens, d_tok_off}, d_part_off, bin_size,
                     nbins, nbits, d_perm, d_bin_id, d_counts);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_bin_stable(lddl_ctx* c, void* stream, const int32_t* d_num_tokens,
                               const int64_t* d_tok_off, int64_t n_rows, int32_t bin_size,
                               int32_t nbins, int64_t* d_perm, int64_t* d_bin_id, int64_t* d_counts) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (bin_size < 1 || nbins < 1) LDDL_FAIL(-1, "bin_size and nbins must be >= 1");
  if (nbins > kMaxBinsLds) LDDL_FAIL(-1, "nbins %d > %d unsupported", nbins, kMaxBinsLds);
  if (n_rows < 0) LDDL_FAIL(-1, "bad sizes");
  if (!d_num_tokens && !d_tok_off && n_rows) LDDL_FAIL(-1, "need num_tokens or tok_off");
  hipStream_t st = as_stream(stream);
  if (n_rows == 0) {
    LDDL_HIP(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * nbins, st));
    return 0;
  }
  const NumTok nt{d_num_tokens, d_tok_off};
  int nbits = 0;
  while ((1 << nbits) < nbins) ++nbits;
  const int64_t n_tiles = (n_rows + kBinTile - 1) / kBinTile;
  const int64_t m = n_tiles * nbins;
  ArenaTmp tcb(&c->arena, st), scb(&c->arena, st);
  LDDL_HIP(tcb.take(sizeof(int64_t) * (2 * m + 1)));
  LDDL_HIP(scb.take(sizeof(int64_t) * scan_scratch_elems(m)));
  int64_t* tc = tcb.as<int64_t>();
  int64_t* base = tc + m;
  hipLaunchKernelGGL(bin_tile_hist_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, nt,
                     n_rows, bin_size, nbins, n_tiles, tc);
  struct In {
    const int64_t* v;
    __device__ int64_t operator()(int64_t i) const { return v[i]; }
  };
  LDDL_HIP(scan_exclusive(In{tc}, m, base, scb.as<int64_t>(), st));
  hipLaunchKernelGGL(bin_tile_scatter_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st,
                     nt, n_rows, bin_size, nbins, nbits, n_tiles, base, d_perm, d_bin_id);
  hipLaunchKernelGGL(bin_totals_kernel, dim3((unsigned)((nbins + 255) / 256)), dim3(256), 0, st,
                     base, n_tiles, nbins, d_counts);
  LDDL_HIP(hipGetLastError());
  return 0;
}
