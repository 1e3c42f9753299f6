// SentencePiece unigram, byte fallback: a pass over the finished paths, between
// the tile and long passes and the compaction. An alive unknown piece stands for the fused run
// of unknown characters from its byte to the next alive byte or break; every byte of that run
// becomes a piece of its own, byte_ids[byte]. Lane = byte, one wave per 64-byte tile.
//   cover  bit x: byte x lies in such a run. The marks of a tile are its alive bytes and its
//          breaks; a byte is covered iff the last mark at or below it is an alive unknown. The
//          bytes below a tile's first mark take the state of the last mark before the tile,
//          found 64 tiles a step with one ballot. Reads sym and alive_bits, writes `cover` only.
//   apply  alive_bits |= cover, sym[x] = byte_ids[text[x]] on the covered bytes.
// Two launches, because a wave of `cover` reads the sym and alive bits of tiles before its own.
#include "device.h"
#include "unigram_norm.h"

namespace lddl {
namespace {

constexpr int kWaves = 4;

__global__ void __launch_bounds__(64 * kWaves) uni_bytes_cover_kernel(UniWork W, int32_t unk_id, uint64_t* cover) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * kWaves + wave_id();
  if (t >= W.n_tiles) return;  // the whole wave
  const uint64_t A = W.alive_bits[t], B = W.break_bits[t];
  const int64_t x = t * 64 + lane;
  const uint64_t U = ballot(((A >> lane) & 1) && W.sym[x] == unk_id);
  const uint64_t M = A | B;
  bool carry = false;  // an unknown run reaches into the tile
  if (!(M & 1)) {
    for (int64_t w0 = t - 1; w0 >= 0; w0 -= 64) {
      const int64_t w = w0 - lane;
      const uint64_t m = w >= 0 ? (W.alive_bits[w] | W.break_bits[w]) : 0;
      const uint64_t found = ballot(m != 0);
      if (!found) continue;
      const int f = __builtin_ctzll(found);  // the nearest such tile
      const int64_t wf = w0 - f;
      const uint64_t Af = W.alive_bits[wf];
      const int q = 63 - __builtin_clzll(Af | W.break_bits[wf]);
      carry = ((Af >> q) & 1) && W.sym[wf * 64 + q] == unk_id;
      break;
    }
  }
  const uint64_t below = uni_upto(M, lane);
  const bool in_run = below ? (U >> (63 - __builtin_clzll(below))) & 1 : carry;
  const uint64_t C = ballot(in_run && x < W.n_bytes);
  if (lane == 0) cover[t] = C;
}

__global__ void __launch_bounds__(256) uni_bytes_apply_kernel(UniWork W, const int32_t* byte_ids,
                                                              const uint64_t* cover) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= W.n_bytes) return;
  const uint64_t C = cover[x >> 6];
  if ((C >> (x & 63)) & 1) W.sym[x] = byte_ids[W.text[x]];
  if (lane_id() == 0 && C) W.alive_bits[x >> 6] |= C;
}

}  // namespace

hipError_t unigram_launch_bytes(const UniTables& T, const UniWork& W, const int32_t* byte_ids,
                                uint64_t* cover, hipStream_t st) {
  hipLaunchKernelGGL(uni_bytes_cover_kernel, dim3((unsigned)((W.n_tiles + kWaves - 1) / kWaves)),
                     dim3(64 * kWaves), 0, st, W, T.unk_id, cover);
  if (W.n_bytes > 0)
    hipLaunchKernelGGL(uni_bytes_apply_kernel, dim3((unsigned)((W.n_bytes + 255) / 256)), dim3(256), 0, st,
                       W, byte_ids, cover);
  return hipGetLastError();
}

}  // namespace lddl
