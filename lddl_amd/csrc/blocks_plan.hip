// RoBERTa's FULL-SENTENCES / DOC-SENTENCES block cut over a whole round of sentences (DESIGN
// §30; include/lddl_amd.h states the semantics). A block's start depends on every block before
// it, so the cut is one chain b_{k+1} = next(b_k) through all sentences. It is walked on two
// levels: inside a tile of kBlkTile sentences by pointer doubling in LDS, across the tiles by
// one wave that takes one dependent load per tile.
//
//   sep      sep(s): a thread per document walks back from its end to the last sentence that
//            holds a piece (FULL mode; DOC mode only clears)
//   costs    one scan_exclusive over c(s) = min(len + sep, T) -> P[n_sent + 1]
//   tile     a workgroup per tile: P of the tile (and its end) staged in LDS; next(i) by
//            bisection, in LDS when P[tile end] > P[i] + T, else in global P (a run of empty
//            sentences makes the distance unbounded); J[i] = next(i) inside the tile, i itself
//            when next(i) leaves it; kBlkRounds doublings J = J o J with a barrier each give the
//            chain's last element inside the tile, and exit(i) = next of that one
//   chain    one wave: e = 0; entry[tile of e] = e; e = exit[e]: n_sent / kBlkTile dependent
//            loads. The tile pass left entry = -1 in every tile, so a tile the chain jumps over
//            keeps it
//   mark     a workgroup per tile with an entry: J again from the stored next, R = {entry},
//            kBlkRounds rounds of R |= J(R), J = J o J; flag[s] = s is in R and its block holds a
//            piece; the tile's count
//   write    a scan_exclusive of the counts over the tiles; a workgroup per tile ranks its flags
//            (block_excl_scan) and writes block_sent / block_len in order
//
// No host wait, no atomics; the temporaries (next, exit, entry, flags, counts: 17 bytes a
// sentence) come from a DevArena that this unit owns per device.
#include <map>
#include <mutex>

#include "arena.h"
#include "blocks_dev.h"
#include "common.h"
#include "ctx.h"
#include "scan.h"

namespace lddl {
namespace {

struct PlanArgs {
  const int32_t* sent_len;
  const int64_t* dso;  // doc_sent_off[n_doc + 1]
  int64_t n_sent, n_doc;
  int32_t T, mode;
  uint8_t* sep;          // [n_sent]
  int64_t* P;            // [n_sent + 1]
  int64_t* next;         // [n_sent]
  int64_t* exit;         // [n_sent]
  int64_t* entry;        // [n_tiles]
  uint8_t* flag;         // [n_tiles * kBlkTile]
  int64_t* tile_count;   // [n_tiles]
  int64_t* tile_base;    // [n_tiles + 1]
  int64_t* block_sent;   // [n_sent + 1]
  int32_t* block_len;    // [n_sent + 1]
  int64_t* n_blocks;     // [1]
};

__device__ inline int64_t clamp_sent(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

__global__ void __launch_bounds__(256) blocks_sep_clear_kernel(PlanArgs A) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < A.n_sent) A.sep[s] = 0;
}

// the last sentence of non-zero length of document d takes the separator
__global__ void __launch_bounds__(256) blocks_sep_mark_kernel(PlanArgs A) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= A.n_doc) return;
  const int64_t a = clamp_sent(A.dso[d], A.n_sent);
  int64_t s = clamp_sent(A.dso[d + 1], A.n_sent) - 1;
  while (s >= a && (A.sent_len[s] & kLenMask) == 0) --s;
  if (s >= a) A.sep[s] = 1;
}

// the end of sentence i's document: the first entry of doc_sent_off above i (n_sent if none)
__device__ inline int64_t doc_end(const PlanArgs& A, int64_t i) {
  int64_t lo = -1, hi = A.n_doc + 1;  // dso[lo] <= i < dso[hi], the ends as sentinels
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (A.dso[mid] <= i) lo = mid;
    else hi = mid;
  }
  return hi <= A.n_doc ? clamp_sent(A.dso[hi], A.n_sent) : A.n_sent;
}

// J = J o J, kBlkRounds times; every thread of the workgroup calls it
__device__ inline void double_jumps(int32_t* J, int32_t n) {
  for (int r = 0; r < kBlkRounds; ++r) {
    int32_t v[kBlkItems];
#pragma unroll
    for (int k = 0; k < kBlkItems; ++k) {
      const int32_t i = threadIdx.x + k * kBlkThreads;
      v[k] = i < n ? J[J[i]] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBlkItems; ++k) {
      const int32_t i = threadIdx.x + k * kBlkThreads;
      if (i < n) J[i] = v[k];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlkThreads) blocks_tile_kernel(PlanArgs A) {
  __shared__ int64_t Pl[kBlkTile + 1];  // P of the tile and its end; then next, for the exits
  __shared__ int32_t J[kBlkTile];
  const int64_t base = (int64_t)blockIdx.x * kBlkTile;
  const int64_t left = A.n_sent - base;
  const int32_t n = (int32_t)(left < kBlkTile ? left : kBlkTile);
  for (int32_t j = threadIdx.x; j <= n; j += kBlkThreads) Pl[j] = A.P[base + j];
  if (threadIdx.x == 0) A.entry[blockIdx.x] = -1;
  __syncthreads();
  const int64_t p_end = Pl[n];
  int64_t nx[kBlkItems];
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    const int32_t i = threadIdx.x + k * kBlkThreads;
    nx[k] = 0;
    if (i < n) {
      const int64_t target = Pl[i] + A.T;
      int64_t j;
      if (p_end > target) {  // inside the tile: Pl[i + 1] <= target (c <= T) and Pl[n] > target
        int32_t lo = i + 1, hi = n;
        while (hi - lo > 1) {
          const int32_t mid = (lo + hi) >> 1;
          if (Pl[mid] <= target) lo = mid;
          else hi = mid;
        }
        j = base + lo;
      } else {  // at or past the tile's end: P[base + n] <= target
        int64_t lo = base + n, hi = A.n_sent + 1;
        while (hi - lo > 1) {
          const int64_t mid = lo + (hi - lo) / 2;
          if (A.P[mid] <= target) lo = mid;
          else hi = mid;
        }
        j = lo;
      }
      if (A.mode == LDDL_BLOCKS_DOC) {
        const int64_t e = doc_end(A, base + i);
        j = j < e ? j : e;
      }
      nx[k] = j;
    }
  }
  __syncthreads();  // Pl is dead: it takes next
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    const int32_t i = threadIdx.x + k * kBlkThreads;
    if (i < n) {
      Pl[i] = nx[k];
      J[i] = nx[k] - base < n ? (int32_t)(nx[k] - base) : i;
    }
  }
  __syncthreads();
  double_jumps(J, n);  // J[i]: the chain's last element inside the tile
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    const int32_t i = threadIdx.x + k * kBlkThreads;
    if (i < n) {
      A.next[base + i] = nx[k];
      A.exit[base + i] = Pl[J[i]];
    }
  }
}

// exit[e] > e; a value that is not ends the walk instead of hanging it
__global__ void __launch_bounds__(64) blocks_chain_kernel(PlanArgs A) {
  int64_t e = 0;
  while (e < A.n_sent) {
    if (lane_id() == 0) A.entry[e / kBlkTile] = e;
    const int64_t ne = A.exit[e];
    e = ne > e ? ne : A.n_sent;
  }
}

__global__ void __launch_bounds__(kBlkThreads) blocks_mark_kernel(PlanArgs A) {
  __shared__ int32_t J[kBlkTile];
  __shared__ uint8_t R[kBlkTile];
  const int64_t base = (int64_t)blockIdx.x * kBlkTile;
  const int64_t left = A.n_sent - base;
  const int32_t n = (int32_t)(left < kBlkTile ? left : kBlkTile);
  const int64_t e = A.entry[blockIdx.x];
  if (e < base || e >= base + n) {  // the whole workgroup: the chain jumps over the tile
    for (int32_t i = threadIdx.x; i < kBlkTile; i += kBlkThreads) A.flag[base + i] = 0;
    if (threadIdx.x == 0) A.tile_count[blockIdx.x] = 0;
    return;
  }
  int64_t nx[kBlkItems];
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    const int32_t i = threadIdx.x + k * kBlkThreads;
    nx[k] = i < n ? A.next[base + i] : 0;
    if (i < n) J[i] = nx[k] - base < n ? (int32_t)(nx[k] - base) : i;
    R[i] = base + i == e ? 1 : 0;
  }
  __syncthreads();
  // R |= J(R), J = J o J: after round r, R holds the chain's first 2^(r + 1) elements at least,
  // and only elements of the chain (a lane that sees a mark of this round early marks one more)
  for (int r = 0; r < kBlkRounds; ++r) {
    int32_t v[kBlkItems];
#pragma unroll
    for (int k = 0; k < kBlkItems; ++k) {
      const int32_t i = threadIdx.x + k * kBlkThreads;
      v[k] = 0;
      if (i < n) {
        const int32_t j = J[i];
        if (R[i]) R[j] = 1;
        v[k] = J[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBlkItems; ++k) {
      const int32_t i = threadIdx.x + k * kBlkThreads;
      if (i < n) J[i] = v[k];
    }
    __syncthreads();
  }
  int64_t cnt = 0;
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    const int32_t i = threadIdx.x + k * kBlkThreads;
    const bool f = i < n && R[i] && A.P[clamp_sent(nx[k], A.n_sent)] > A.P[base + i];
    A.flag[base + i] = f ? 1 : 0;
    cnt += f ? 1 : 0;
  }
  int64_t tot;
  block_excl_scan(cnt, &tot);
  if (threadIdx.x == 0) A.tile_count[blockIdx.x] = tot;
}

struct BlockTileCount {
  const int64_t* count;
  __device__ int64_t operator()(int64_t t) const { return count[t]; }
};

// thread t ranks the kBlkItems consecutive sentences from t * kBlkItems
__global__ void __launch_bounds__(kBlkThreads) blocks_write_kernel(PlanArgs A) {
  static_assert(kBlkThreads == kScanThreads, "block_excl_scan's workgroup");
  const int64_t first = (int64_t)blockIdx.x * kBlkTile + (int64_t)threadIdx.x * kBlkItems;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t total = A.tile_base[gridDim.x];
    A.block_sent[total] = A.n_sent;
    A.n_blocks[0] = total;
  }
  bool f[kBlkItems];
  int64_t cnt = 0;
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    f[k] = A.flag[first + k] != 0;  // (the flags cover whole tiles)
    cnt += f[k] ? 1 : 0;
  }
  int64_t tot;
  int64_t at = A.tile_base[blockIdx.x] + block_excl_scan(cnt, &tot);
#pragma unroll
  for (int k = 0; k < kBlkItems; ++k) {
    if (f[k] && at <= A.n_sent) {
      const int64_t s = first + k;
      A.block_sent[at] = s;
      A.block_len[at] = (int32_t)(A.P[clamp_sent(A.next[s], A.n_sent)] - A.P[s]);
      ++at;
    }
  }
}

__global__ void blocks_none_kernel(PlanArgs A) {
  A.P[0] = 0;
  A.block_sent[0] = 0;
  A.n_blocks[0] = 0;
}

// The arena of the plan's temporaries, one per device, for the life of the process (the plan
// has no context to own it; lddl_blocks_release returns its memory).
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

extern "C" int lddl_blocks_plan(void* stream, const int32_t* d_sent_len, int64_t n_sent,
                                const int64_t* d_doc_sent_off, int64_t n_doc, int32_t seq_len,
                                int32_t mode, int64_t* d_piece_off, uint8_t* d_sent_sep,
                                int64_t* d_block_sent, int32_t* d_block_len,
                                int64_t* d_n_blocks) {
  if (seq_len < 3 || seq_len > (1 << 24))
    LDDL_FAIL(-1, "seq_len %d: a row holds bos, a piece and eos at least, 2^24 slots at most",
              seq_len);
  if (mode != LDDL_BLOCKS_FULL && mode != LDDL_BLOCKS_DOC)
    LDDL_FAIL(-1, "mode %d is neither LDDL_BLOCKS_FULL nor LDDL_BLOCKS_DOC", mode);
  if (n_sent < 0 || n_doc < 0) LDDL_FAIL(-1, "negative size");
  if (!d_piece_off || !d_block_sent || !d_block_len || !d_n_blocks) LDDL_FAIL(-1, "null output");
  if (n_sent > 0 && (!d_sent_len || !d_doc_sent_off || !d_sent_sep))
    LDDL_FAIL(-1, "null token table");
  hipStream_t st = as_stream(stream);
  PlanArgs A{};
  A.sent_len = d_sent_len;
  A.dso = d_doc_sent_off;
  A.n_sent = n_sent;
  A.n_doc = n_doc;
  A.T = seq_len - 2;
  A.mode = mode;
  A.sep = d_sent_sep;
  A.P = d_piece_off;
  A.block_sent = d_block_sent;
  A.block_len = d_block_len;
  A.n_blocks = d_n_blocks;
  if (n_sent == 0) {
    hipLaunchKernelGGL(blocks_none_kernel, dim3(1), dim3(1), 0, st, A);
    LDDL_HIP(hipGetLastError());
    return 0;
  }
  const int64_t n_tiles = (n_sent + kBlkTile - 1) / kBlkTile;
  DevArena* arena = plan_arena();
  if (!arena) LDDL_FAIL(-100, "no current device");
  ArenaScope tmp(arena, st);
  // one block of int64: next | exit | entry | tile_count | tile_base | the scans' scratch
  const int64_t scratch = scan_scratch_elems(n_sent);
  int64_t* words;
  if (tmp.take(&words, 2 * n_sent + 3 * n_tiles + 1 + scratch)) return -100;
  if (tmp.take(&A.flag, n_tiles * kBlkTile)) return -100;
  A.next = words;
  A.exit = A.next + n_sent;
  A.entry = A.exit + n_sent;
  A.tile_count = A.entry + n_tiles;
  A.tile_base = A.tile_count + n_tiles;
  int64_t* scan_tmp = A.tile_base + n_tiles + 1;
  const unsigned tiles = (unsigned)n_tiles;
  hipLaunchKernelGGL(blocks_sep_clear_kernel, dim3((unsigned)((n_sent + 255) / 256)), dim3(256), 0,
                     st, A);
  if (mode == LDDL_BLOCKS_FULL && n_doc > 0)
    hipLaunchKernelGGL(blocks_sep_mark_kernel, dim3((unsigned)((n_doc + 255) / 256)), dim3(256), 0,
                       st, A);
  LDDL_HIP(scan_exclusive(BlockCost{d_sent_len, d_sent_sep, A.T}, n_sent, A.P, scan_tmp, st));
  hipLaunchKernelGGL(blocks_tile_kernel, dim3(tiles), dim3(kBlkThreads), 0, st, A);
  hipLaunchKernelGGL(blocks_chain_kernel, dim3(1), dim3(64), 0, st, A);
  hipLaunchKernelGGL(blocks_mark_kernel, dim3(tiles), dim3(kBlkThreads), 0, st, A);
  LDDL_HIP(scan_exclusive(BlockTileCount{A.tile_count}, n_tiles, A.tile_base, scan_tmp, st));
  hipLaunchKernelGGL(blocks_write_kernel, dim3(tiles), dim3(kBlkThreads), 0, st, A);
  LDDL_HIP(hipGetLastError());
  return 0;
}

extern "C" int lddl_blocks_release(void) {
  std::lock_guard<std::mutex> g(g_mu);
  for (auto& kv : g_arenas) kv.second->trim();
  return 0;
}
