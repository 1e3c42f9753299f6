// Row movement of the load balance (lddl_amd/balance.py): take, ragged gather and its offsets,
// segmented index expansion, and the packed per-row metadata of the exchange.
// Rows are addressed over two sources: row r < n_a is row r of source A, else row r - n_a of
// source B (a rank's own table and the rows it received), so the exchange never concatenates.
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "scan.h"

namespace lddl {
namespace {

template <typename T>
struct Src2 {
  const T* a;
  const T* b;
  int64_t n_a;
  __device__ const T* at(int64_t r) const { return r < n_a ? a + r : b + (r - n_a); }
};

template <typename T>
__global__ void __launch_bounds__(256) gather_ragged_kernel(Src2<T> src, Src2<int64_t> off,
                                                            const int64_t* __restrict__ rows,
                                                            int64_t n_rows,
                                                            const int64_t* __restrict__ dst_off,
                                                            T* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 4 + wave_id();
  if (i >= n_rows) return;
  const int64_t r = rows ? rows[i] : i;
  const int64_t* o2 = off.at(r);
  const int64_t a = o2[0], n = o2[1] - a, o = dst_off[i];
  const T* s = r < src.n_a ? src.a : src.b;  // offsets are relative to the row's own source
  for (int64_t j = lane_id(); j < n; j += 64) dst[o + j] = s[a + j];
}

template <typename T>
__global__ void __launch_bounds__(256) take_kernel(Src2<T> src, const int64_t* __restrict__ rows,
                                                   int64_t n_rows, T* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_rows) dst[i] = *src.at(rows ? rows[i] : i);
}

// Segmented index expansion: segment k covers outputs [seg_off[k], seg_off[k+1]); its element t
// is v = start + t * stride, written as v (mode 1) or src[v] (mode 0). One thread per output;
// the segment is found by binary search over the (L2-resident) segment offsets.
__global__ void __launch_bounds__(256) expand_segments_kernel(const int64_t* __restrict__ src,
                                                              const int64_t* __restrict__ seg,
                                                              const int64_t* __restrict__ seg_off,
                                                              int64_t n_seg, int64_t total,
                                                              int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int64_t lo = 0, hi = n_seg;  // seg_off[lo] <= i < seg_off[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (seg_off[mid] <= i) lo = mid;
    else hi = mid;
  }
  const int64_t v = seg[3 * lo] + (i - seg_off[lo]) * seg[3 * lo + 1];
  out[i] = seg[3 * lo + 2] ? v : src[v];
}

// Per-row metadata of the exchange: {len(A) + len(B), len(A), is_random_next, masks} as int32[4]
__global__ void __launch_bounds__(256) pairs_meta_pack_kernel(
    const int64_t* __restrict__ tok_off, const int32_t* __restrict__ len_a,
    const uint8_t* __restrict__ is_rn, const int64_t* __restrict__ pos_off,
    const int64_t* __restrict__ rows, int64_t n, int4* __restrict__ meta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows ? rows[i] : i;
  meta[i] = make_int4((int32_t)(tok_off[r + 1] - tok_off[r]), len_a[r], (int32_t)is_rn[r],
                      pos_off ? (int32_t)(pos_off[r + 1] - pos_off[r]) : 0);
}

__global__ void __launch_bounds__(256) pairs_meta_unpack_kernel(
    const int4* __restrict__ meta, int64_t n, int64_t* __restrict__ ntok,
    int32_t* __restrict__ len_a, uint8_t* __restrict__ is_rn, int64_t* __restrict__ nmask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 m = meta[i];
  ntok[i] = m.x;
  len_a[i] = m.y;
  is_rn[i] = (uint8_t)m.z;
  if (nmask) nmask[i] = m.w;
}

// elements of output row i (lddl_ragged_offsets scans it)
struct RowSize {
  Src2<int64_t> off;
  const int64_t* rows;
  __device__ int64_t operator()(int64_t i) const {
    const int64_t* o = off.at(rows ? rows[i] : i);
    return o[1] - o[0];
  }
};

}  // namespace
}  // namespace lddl

using namespace lddl;

// f(T()) with T the unsigned integer of elem_bytes bytes; an unsupported size fails
template <typename F>
static int by_elem_bytes(int32_t elem_bytes, F f) {
  switch (elem_bytes) {
    case 1: f(uint8_t()); break;
    case 2: f(uint16_t()); break;
    case 4: f(uint32_t()); break;
    case 8: f(uint64_t()); break;
    default: LDDL_FAIL(-1, "elem_bytes %d unsupported", elem_bytes);
  }
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_gather_ragged(void* stream, const void* d_src_a, const int64_t* d_off_a,
                                  int64_t n_a, const void* d_src_b, const int64_t* d_off_b,
                                  int32_t elem_bytes, const int64_t* d_rows, int64_t n_rows,
                                  const int64_t* d_dst_off, void* d_dst) {
  if (n_rows < 0 || n_a < 0) LDDL_FAIL(-1, "bad size");
  if (n_rows == 0) return 0;
  if (!d_rows && n_rows > n_a) LDDL_FAIL(-1, "n_rows > n_a without a row index");
  return by_elem_bytes(elem_bytes, [&](auto e) {
    typedef decltype(e) T;
    hipLaunchKernelGGL(gather_ragged_kernel<T>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                       as_stream(stream), Src2<T>{(const T*)d_src_a, (const T*)d_src_b, n_a},
                       Src2<int64_t>{d_off_a, d_off_b, n_a}, d_rows, n_rows, d_dst_off, (T*)d_dst);
  });
}

extern "C" int lddl_take(void* stream, const void* d_a, int64_t n_a, const void* d_b,
                         int32_t elem_bytes, const int64_t* d_rows, int64_t n_rows, void* d_dst) {
  if (n_rows < 0 || n_a < 0) LDDL_FAIL(-1, "bad size");
  if (n_rows == 0) return 0;
  if (!d_rows && n_rows > n_a) LDDL_FAIL(-1, "n_rows > n_a without a row index");
  return by_elem_bytes(elem_bytes, [&](auto e) {
    typedef decltype(e) T;
    hipLaunchKernelGGL(take_kernel<T>, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                       as_stream(stream), Src2<T>{(const T*)d_a, (const T*)d_b, n_a}, d_rows, n_rows, (T*)d_dst);
  });
}

extern "C" int lddl_expand_segments(void* stream, const int64_t* d_src, const int64_t* d_seg,
                                    const int64_t* d_seg_off, int64_t n_seg, int64_t total,
                                    int64_t* d_out) {
  if (n_seg < 0 || total < 0) LDDL_FAIL(-1, "bad size");
  if (total == 0) return 0;
  if (n_seg == 0) LDDL_FAIL(-1, "no segments for %lld outputs", (long long)total);
  hipLaunchKernelGGL(expand_segments_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     as_stream(stream), d_src, d_seg, d_seg_off, n_seg, total, d_out);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_ragged_offsets(lddl_ctx* c, void* stream, const int64_t* d_off_a, int64_t n_a,
                                   const int64_t* d_off_b, const int64_t* d_rows, int64_t n_rows,
                                   int64_t* d_out) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (n_rows < 0 || n_a < 0) LDDL_FAIL(-1, "bad size");
  if (!d_rows && n_rows > n_a) LDDL_FAIL(-1, "n_rows > n_a without a row index");
  hipStream_t st = as_stream(stream);
  ArenaTmp scratch(&c->arena, st);
  LDDL_HIP(scratch.take(sizeof(int64_t) * scan_scratch_elems(n_rows)));
  LDDL_HIP(scan_exclusive(RowSize{Src2<int64_t>{d_off_a, d_off_b, n_a}, d_rows}, n_rows, d_out,
                          scratch.as<int64_t>(), st));
  return 0;
}

extern "C" int lddl_pairs_meta_pack(void* stream, const int64_t* d_tok_off, const int32_t* d_len_a,
                                    const uint8_t* d_is_rn, const int64_t* d_pos_off,
                                    const int64_t* d_rows, int64_t n, int32_t* d_meta) {
  if (n < 0) LDDL_FAIL(-1, "bad size");
  if (n == 0) return 0;
  hipLaunchKernelGGL(pairs_meta_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), d_tok_off, d_len_a, d_is_rn, d_pos_off, d_rows, n,
                     reinterpret_cast<int4*>(d_meta));
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_pairs_meta_unpack(void* stream, const int32_t* d_meta, int64_t n,
                                      int64_t* d_ntok, int32_t* d_len_a, uint8_t* d_is_rn,
                                      int64_t* d_nmask) {
  if (n < 0) LDDL_FAIL(-1, "bad size");
  if (n == 0) return 0;
  hipLaunchKernelGGL(pairs_meta_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     as_stream(stream), reinterpret_cast<const int4*>(d_meta), n, d_ntok, d_len_a,
                     d_is_rn, d_nmask);
  LDDL_HIP(hipGetLastError());
  return 0;
}
