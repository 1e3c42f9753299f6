// Sample table -> output layout on the GPU, second step: the string / npy rendering of the
// parquet columns (binning is output_bin.hip).
//
// Reference:
//   instance dict                  lddl/dask/bert/pretrain.py:345-358 -> render_*_kernel
//     A / B = ' '.join(tokens), masked_lm_labels = ' '.join(labels),
//     masked_lm_positions = serialize_np_array(uint16[k]) (lddl/utils.py:98-102: np.save bytes,
//     a fixed 128-byte v1.0 header then 2k little-endian bytes).
//
// render: one wavefront per row. Lane j owns token j of a 64-token chunk; its string length
// comes from the vocab render table, a wave scan gives byte offsets, and each lane copies its
// token string and the separating space.
#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"

namespace lddl {
namespace {

struct RenderArgs {
  const uint8_t* rbytes;  // vocab render table
  const int64_t* roff;
  const void* tokens;  // ids of lddl_ctx::id_bytes bytes each (uint16 or int32)
  const int64_t* tok_off;
  const int32_t* len_a;
  const uint16_t* pos;
  const void* lab;     // as tokens
  const int64_t* pos_off;
  const int64_t* rows;  // output row -> pair (NULL: identity)
  int64_t n_rows;
  int32_t ib;           // bytes per id
};

// id i of an id array of R.ib-byte entries
__device__ inline int32_t id_at(const RenderArgs& R, const void* ids, int64_t i) {
  return R.ib == 2 ? (int32_t)static_cast<const uint16_t*>(ids)[i] : static_cast<const int32_t*>(ids)[i];
}

__device__ inline int32_t tok_len(const RenderArgs& R, int32_t id) {
  return (int32_t)(R.roff[id + 1] - R.roff[id]);
}

// total bytes of ' '.join(strings of ids[i0 .. i0 + n))
__device__ int64_t joined_len(const RenderArgs& R, const void* ids, int64_t i0, int64_t n) {
  int64_t acc = 0;
  for (int64_t c0 = 0; c0 < n; c0 += 64) {
    const int64_t j = c0 + lane_id();
    acc += j < n ? tok_len(R, id_at(R, ids, i0 + j)) : 0;
  }
  return wave_sum(acc) + (n > 0 ? n - 1 : 0);
}

__device__ void joined_write(const RenderArgs& R, const void* ids, int64_t i0, int64_t n,
                             uint8_t* out) {
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < n; c0 += 64) {
    const int64_t j = c0 + lane_id();
    const int32_t id = j < n ? id_at(R, ids, i0 + j) : 0;
    const int64_t l = j < n ? tok_len(R, id) + 1 : 0;  // string + separator
    const int64_t incl = wave_incl_scan(l);
    if (j < n) {
      uint8_t* o = out + base + incl - l;
      const uint8_t* src = R.rbytes + R.roff[id];
      for (int64_t q = 0; q < l - 1; ++q) o[q] = src[q];
      if (j < n - 1) o[l - 1] = ' ';
    }
    base += __shfl(incl, 63, 64);
  }
}

__global__ void __launch_bounds__(256) render_lengths_kernel(RenderArgs R, int64_t* a_len,
                                                             int64_t* b_len, int64_t* l_len,
                                                             int64_t* n_pos, const uint8_t* is_rn,
                                                             uint16_t* num_tokens_out,
                                                             uint8_t* is_rn_out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
  if (row >= R.n_rows) return;
  const int64_t q = R.rows ? R.rows[row] : row;
  const int64_t t0 = R.tok_off[q], t1 = R.tok_off[q + 1];
  const int32_t na = R.len_a[q];
  const int64_t la = joined_len(R, R.tokens, t0, na);
  const int64_t lb = joined_len(R, R.tokens, t0 + na, t1 - t0 - na);
  int64_t ll = 0, np = 0;
  if (R.pos_off) {
    const int64_t p0 = R.pos_off[q], p1 = R.pos_off[q + 1];
    ll = joined_len(R, R.lab, p0, p1 - p0);
    np = p1 - p0;
  }
  if (lane_id() == 0) {
    a_len[row] = la;
    b_len[row] = lb;
    if (l_len) l_len[row] = ll;
    if (n_pos) n_pos[row] = 128 + 2 * np;
    // the row's num_tokens / is_random_next columns in output order
    if (num_tokens_out) num_tokens_out[row] = (uint16_t)(t1 - t0 + 3);
    if (is_rn_out) is_rn_out[row] = is_rn[q];
  }
}

__device__ void put_npy(uint8_t* o, const uint16_t* pos, int64_t k) {
  // 128-byte NPY v1.0 header of a 1-D '<u2' array of length k, as np.save writes it
  const char* pre = "\x93NUMPY\x01\x00v\x00{'descr': '<u2', 'fortran_order': False, 'shape': (";
  const int pre_len = 10 + 51;
  char digits[24];
  int nd = 0;
  int64_t v = k;
  do { digits[nd++] = (char)('0' + v % 10); v /= 10; } while (v);
  const int lane = lane_id();
  for (int i = lane; i < 128; i += 64) {
    char c;
    if (i < pre_len) c = pre[i];
    else if (i < pre_len + nd) c = digits[nd - 1 - (i - pre_len)];
    else if (i < pre_len + nd + 5) c = ",), }"[i - pre_len - nd];
    else if (i < 127) c = ' ';
    else c = '\n';
    o[i] = (uint8_t)c;
  }
  for (int64_t j = lane; j < k; j += 64) {
    o[128 + 2 * j] = (uint8_t)(pos[j] & 0xFF);
    o[128 + 2 * j + 1] = (uint8_t)(pos[j] >> 8);
  }
}

__global__ void __launch_bounds__(256) render_write_kernel(RenderArgs R, const int64_t* a_off,
                                                           const int64_t* b_off, const int64_t* l_off,
                                                           const int64_t* npy_off, uint8_t* a_bytes,
                                                           uint8_t* b_bytes, uint8_t* l_bytes,
                                                           uint8_t* npy_bytes) {
  const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
  if (row >= R.n_rows) return;
  const int64_t q = R.rows ? R.rows[row] : row;
  const int64_t t0 = R.tok_off[q], t1 = R.tok_off[q + 1];
  const int32_t na = R.len_a[q];
  joined_write(R, R.tokens, t0, na, a_bytes + a_off[row]);
  joined_write(R, R.tokens, t0 + na, t1 - t0 - na, b_bytes + b_off[row]);
  if (R.pos_off) {
    const int64_t p0 = R.pos_off[q], p1 = R.pos_off[q + 1];
    if (l_bytes) joined_write(R, R.lab, p0, p1 - p0, l_bytes + l_off[row]);
    if (npy_bytes) put_npy(npy_bytes + npy_off[row], R.pos + p0, p1 - p0);
  }
}

}  // namespace
}  // namespace lddl

using namespace lddl;

static RenderArgs make_render(const lddl_ctx* c, const void* d_tokens, const int64_t* d_tok_off,
                              const int32_t* d_len_a, const uint16_t* d_pos, const void* d_lab,
                              const int64_t* d_pos_off, const int64_t* d_rows, int64_t n_rows) {
  return RenderArgs{c->d_render, c->d_render_off, d_tokens, d_tok_off, d_len_a, d_pos, d_lab,
                    d_pos_off, d_rows, n_rows, c->id_bytes()};
}

extern "C" int lddl_render_lengths(lddl_ctx* c, void* stream, const void* d_tokens,
                                   const int64_t* d_tok_off, const int32_t* d_len_a,
                                   const void* d_lab, const int64_t* d_pos_off,
                                   const int64_t* d_rows, int64_t n_rows, int64_t* d_a_len,
                                   int64_t* d_b_len, int64_t* d_l_len, int64_t* d_npy_len,
                                   const uint8_t* d_is_rn, uint16_t* d_num_tokens_out,
                                   uint8_t* d_is_rn_out) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (n_rows <= 0) return 0;
  if (d_is_rn_out && !d_is_rn) LDDL_FAIL(-1, "is_random_next output without input");
  const RenderArgs R = make_render(c, d_tokens, d_tok_off, d_len_a, nullptr, d_lab, d_pos_off,
                                   d_rows, n_rows);
  hipLaunchKernelGGL(render_lengths_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                     as_stream(stream), R, d_a_len, d_b_len, d_l_len, d_npy_len, d_is_rn,
                     d_num_tokens_out, d_is_rn_out);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_render_write(lddl_ctx* c, void* stream, const void* d_tokens,
                                 const int64_t* d_tok_off, const int32_t* d_len_a,
                                 const uint16_t* d_pos, const void* d_lab,
                                 const int64_t* d_pos_off, const int64_t* d_rows, int64_t n_rows,
                                 const int64_t* d_a_off, const int64_t* d_b_off,
                                 const int64_t* d_l_off, const int64_t* d_npy_off,
                                 uint8_t* d_a_bytes, uint8_t* d_b_bytes, uint8_t* d_l_bytes,
                                 uint8_t* d_npy_bytes) {
  if (!c) LDDL_FAIL(-1, "null ctx");
  if (n_rows <= 0) return 0;
  const RenderArgs R = make_render(c, d_tokens, d_tok_off, d_len_a, d_pos, d_lab, d_pos_off, d_rows,
                                   n_rows);
  hipLaunchKernelGGL(render_write_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0,
                     as_stream(stream), R, d_a_off, d_b_off, d_l_off, d_npy_off, d_a_bytes,
                     d_b_bytes, d_l_bytes, d_npy_bytes);
  LDDL_HIP(hipGetLastError());
  return 0;
}
