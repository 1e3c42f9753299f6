// Pair stage, the dense packing of the kept tokens where no planner launch does it (the stage's
// other units: file map in pairs_api.hip): densify_kernel over all kept sentences, its variant
// bounded by a device value for the head range of a split replay plan, and their launchers.
#include "densify_dev.h"

namespace lddl {
namespace {

// Kept tokens packed densely in kept-sentence order: kept sentence k's pieces are
// dense[kscan[k] .. kscan[k+1]). A pair's A (and B) window is then one contiguous run
// dense[kscan[a_ks] + a_front ..+ na), because a span only ever covers consecutive kept
// sentences of one document. One wave per 64 kept sentences; 64-token output chunks are stored
// coalesced, each lane finding its sentence among the few that overlap the chunk.
__global__ void __launch_bounds__(256) densify_kernel(const int64_t* __restrict__ ks_start,
                                                      const int32_t* __restrict__ ks_len,
                                                      const int64_t* __restrict__ kscan, int64_t n,
                                                      const int32_t* __restrict__ ids,
                                                      IdPtr dense) {
  const int64_t k0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 64;
  if (k0 >= n) return;
  densify_group(k0, ks_start, ks_len, kscan, n, ids, dense);
}

// densify_kernel over kept sentences [0, *n_ptr): the head range of a split plan (the launch
// covers all kept sentences; the workgroups past the bound leave at once)
__global__ void __launch_bounds__(256) densify_head_kernel(const int64_t* __restrict__ ks_start,
                                                           const int32_t* __restrict__ ks_len,
                                                           const int64_t* __restrict__ kscan,
                                                           const int64_t* __restrict__ n_ptr,
                                                           const int32_t* __restrict__ ids,
                                                           IdPtr dense) {
  const int64_t n = *n_ptr;
  const int64_t k0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 64;
  if (k0 >= n) return;
  densify_group(k0, ks_start, ks_len, kscan, n, ids, dense);
}

}  // namespace

// densify_kernel over all kept sentences (n > 0), its one launch site: compact_inputs packs
// `dense` with it when no planner launch does, launch_planner for a sliced plan that asks for it
// (LDDL_PLAN_SLICE_DENSE)
void launch_densify(const int64_t* ks_start, const int32_t* ks_len, const int64_t* kscan, int64_t n,
                    const int32_t* ids, IdPtr dense, hipStream_t st) {
  hipLaunchKernelGGL(densify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ks_start,
                     ks_len, kscan, n, ids, dense);
}

// densify_head_kernel, its one launch site (plan_replay_split_head): a grid over all n > 0 kept
// sentences, of which those below *n_ptr (split_info_kernel's info[0]) are packed
void launch_densify_head(const int64_t* ks_start, const int32_t* ks_len, const int64_t* kscan, int64_t n,
                         const int64_t* n_ptr, const int32_t* ids, IdPtr dense, hipStream_t st) {
  hipLaunchKernelGGL(densify_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ks_start,
                     ks_len, kscan, n_ptr, ids, dense);
}

}  // namespace lddl
