// Pair stage, the native planner (LDDL_RNG_NATIVE): the reference's algorithms on counter-based
// Philox streams, its two mask kernels (plain and whole-word) and the keyed partition order.
#include "collate_dev.h"  // ContBits, cont_id
#include "pairs_plan.h"

// (scan functor over the masks per pair; at file scope, where it has always been: the scan
// kernels instantiated over it keep their names)
struct I32 {
  const int32_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i]; }
};

namespace lddl {
namespace {

// ---------------------------------------------------------------------------------------------
// Native RNG mode (LDDL_RNG_NATIVE): the same algorithms (create_pairs_from_document,
// _truncate_seq_pair, create_masked_lm_predictions, the partition shuffle) drawing from
// Philox4x32-10 instead of one sequential MT19937 per partition, so every (duplicate, document)
// walk and every pair's masking runs in its own lane. A stream is keyed by
// (native_seed, part_seed[p]) and counted by the unit's or pair's index inside its partition, so
// a partition's output does not depend on how partitions are batched or sharded.
// Distributions are those of the reference: in the walk, randint / _randbelow by the same
// bit-length rejection and random() < p on the same 53-bit integer, each truncation side a fair
// coin; in the masking, the masked set a uniform num_to_predict-subset of the candidates (Floyd's
// algorithm: the shuffled prefix of pretrain.py:197-207 is a uniform subset) and 80/10/10
// decisions per masked token, both from one 32-bit draw each (exact uniform integers by Lemire's
// multiply-shift with rejection).
// ---------------------------------------------------------------------------------------------
__device__ inline uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ inline uint64_t part_key(uint64_t native_seed, int64_t part_seed) {
  return mix64(native_seed ^ mix64((uint64_t)part_seed + 0x9E3779B97F4A7C15ull));
}

enum : uint32_t { kStreamWalk = 1, kStreamMask = 2, kStreamOrder = 3, kStreamDecide = 4 };

struct CtrRng {
  uint2 key;
  uint32_t id0, id1, blk;
  uint4 buf;
  int have;
  __device__ CtrRng(uint64_t k, int64_t index, uint32_t stream)
      : key{(uint32_t)k, (uint32_t)(k >> 32)},
        id0((uint32_t)index),
        id1((uint32_t)((uint64_t)index >> 32) << 4 | stream),
        blk(0),
        have(0) {}
  __device__ uint32_t u32() {
    if (have == 0) {
      buf = Philox::gen(make_uint4(blk++, id0, id1, 0x6C64646Cu), key);
      have = 4;
    }
    --have;
    return have == 3 ? buf.x : have == 2 ? buf.y : have == 1 ? buf.z : buf.w;
  }
  __device__ uint64_t rand53() {  // the 53-bit integer behind random()
    const uint32_t a = u32() >> 5, b = u32() >> 6;
    return ((uint64_t)a << 26) | b;
  }
  __device__ bool coin() { return u32() < 0x80000000u; }
  __device__ uint32_t randbelow(uint32_t n) {  // _randbelow: k-bit draws until < n
    const int k = 32 - __clz(n);
    uint32_t r = u32() >> (32 - k);
    while (r >= n) r = u32() >> (32 - k);
    return r;
  }
  __device__ int64_t randint(int64_t a, int64_t b) { return a + randbelow((uint32_t)(b - a + 1)); }
  __device__ int32_t heads(int32_t n) {  // number of heads in n fair coins
    int32_t h = 0;
    for (; n >= 32; n -= 32) h += __popc(u32());
    if (n > 0) h += __popc(u32() & ((1u << n) - 1u));
    return h;
  }
};

struct NativeArgs {
  const int32_t* ks_len;
  const int64_t* kd_off;
  const int64_t* kp_off;
  const int64_t* kscan;
  IdPtr dense;
  const int64_t* part_seed;
  int64_t n_part, n_units, unit0;  // units dup * (kp_off[0] .. kp_off[n_part])
  uint64_t native_seed, k_short;
  int32_t seq, dup, masking, cls_id, sep_id, mask_id, vocab_size;
  double ratio;
  int64_t* ucnt;        // count pass: pairs of each (duplicate, document) unit
  const int64_t* uoff;  // emit pass: first pair of each unit (exclusive scan of ucnt)
  const int64_t* part_base;
  PairDesc* desc;
  int32_t* nmask;
  int32_t* ncand;
  int32_t* ppart;
  const int64_t* moff;
  uint16_t* mpos;
  int32_t* mtok;
  int64_t* src;
  int64_t n_pairs;
  int32_t words;  // bitmap words per lane (mask kernel)
};

// token t of the window [front, front + n) of the span starting at kept sentence k
__device__ inline int32_t win_token(const NativeArgs& A, int64_t k, int32_t front, int32_t t) {
  return A.dense.ld(A.kscan[k] + front + t);
}

// One partition's walk tables: cumulative kept-sentence lengths and document starts, both
// partition-relative. Staged in LDS when the partition fits (every length sum and search of the
// walk is then an LDS read), else read from the global prefix `g_pre` (int64 over all kept
// sentences) and kd_off. The branch is uniform over the workgroup.
struct WalkTab {
  const int32_t* s_pre;  // [nsp + 1]
  const int32_t* s_doc;  // [nd + 1]
  const int64_t* g_pre;
  const int64_t* g_doc;  // kd_off + d0
  int64_t sb, pre_sb;    // the partition's first kept sentence, g_pre[sb]
  bool lds;
  __device__ int64_t pre(int64_t i) const { return lds ? (int64_t)s_pre[i] : g_pre[sb + i] - pre_sb; }
  __device__ int32_t doc(int64_t d) const { return lds ? s_doc[d] : (int32_t)(g_doc[d] - sb); }
};

// Smallest e in [i, end) whose sentences i..e reach `need` = pre(i) + target (pre(e + 1) >= need),
// else end - 1: the chunk / random-B loops of create_pairs_from_document (pretrain.py:276-280,
// 300-304) as a galloping search over the cumulative lengths (pre(i) < need on entry).
__device__ inline int32_t first_reaching(const WalkTab& W, int32_t i, int32_t end, int64_t need) {
  int32_t a = i, b = i + 1;
  for (int32_t step = 1;; step <<= 1) {
    b = a + step;
    if (b >= end) {
      b = end;
      break;
    }
    if (W.pre(b) >= need) break;
    a = b;
  }
  if (b == end && W.pre(end) < need) return end - 1;
  while (b - a > 1) {  // pre(a) < need <= pre(b)
    const int32_t m = (a + b) >> 1;
    if (W.pre(m) >= need) b = m;
    else a = m;
  }
  return b - 1;
}

// Literal [CLS]/[SEP] among kept sentences [x, y) of the partition (rare: only partitions that
// hold one at all look).
__device__ inline int32_t range_flags(const NativeArgs& A, bool has_flags, int64_t sb, int32_t x,
                                      int32_t y) {
  int32_t f = 0;
  if (has_flags)
    for (int32_t j = x; j < y; ++j) f |= A.ks_len[sb + j];
  return f & kLenHasClsSep;
}

constexpr int kNativeThreads = 256;

// Unit r = (duplicate dp, document dl) of partition p is r = dp * nd + dl (the reference's
// `for _ in range(dup): for doc in docs` order); its global index is dup * (kp_off[p] -
// kp_off[0]) + r. One workgroup per partition: the partition's cumulative sentence lengths and
// document starts are staged in LDS, then every lane walks units, one chunk (pair) per loop
// iteration, taking the partition's next unit from an LDS counter when its unit ends - so a lane
// whose document is short does not idle while another lane's runs on. Chunk ends, A/B lengths and
// the random-next B span are LDS searches over the cumulative lengths (no per-sentence loop).
// EMIT = false counts each unit's pairs; EMIT = true replays the identical draws and writes them
// at uoff[unit].
template <bool EMIT>
__global__ void __launch_bounds__(kNativeThreads) plan_native_kernel(NativeArgs A, const int64_t* g_pre,
                                                                     int32_t lds_words) {
  extern __shared__ int32_t s_tab[];
  __shared__ int32_t s_next;
  const int64_t p = blockIdx.x;
  const int64_t d0 = A.kp_off[p], nd = A.kp_off[p + 1] - d0;
  const int64_t sb = A.kd_off[d0], nsp = A.kd_off[d0 + nd] - sb;
  WalkTab W{s_tab, s_tab + nsp + 1, g_pre, A.kd_off + d0, sb, 0,
            nsp + nd + 2 <= (int64_t)lds_words};
  bool flag_any = false;
  if (W.lds) {
    int32_t* pre = s_tab;
    int32_t* dst = s_tab + nsp + 1;
    for (int64_t i = threadIdx.x; i < nsp; i += kNativeThreads) {
      const int32_t v = A.ks_len[sb + i];
      pre[i + 1] = v & kLenMask;
      flag_any |= (v & kLenHasClsSep) != 0;
    }
    for (int64_t d = threadIdx.x; d <= nd; d += kNativeThreads) dst[d] = (int32_t)(A.kd_off[d0 + d] - sb);
    if (threadIdx.x == 0) {
      pre[0] = 0;
      s_next = kNativeThreads;
    }
    __syncthreads();
    // in-place inclusive scan of pre[1 .. nsp]: a contiguous run per thread, then the runs' sums
    const int32_t per = (int32_t)((nsp + kNativeThreads - 1) / kNativeThreads);
    const int32_t x0 = 1 + (int32_t)threadIdx.x * per;
    const int32_t x1 = min(x0 + per, (int32_t)nsp + 1);
    int32_t run = 0;
    for (int32_t x = x0; x < x1; ++x) run += pre[x];
    __shared__ int32_t s_wsum[kNativeThreads / 64];
    const int32_t inc = wave_incl_scan(run);
    if ((threadIdx.x & 63) == 63) s_wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    int32_t off = inc - run;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += s_wsum[w];
    for (int32_t x = x0; x < x1; ++x) {
      off += pre[x];
      pre[x] = off;
    }
  } else {
    W.pre_sb = g_pre[sb];
    for (int64_t i = threadIdx.x; i < nsp; i += kNativeThreads)
      flag_any |= (A.ks_len[sb + i] & kLenHasClsSep) != 0;
    if (threadIdx.x == 0) s_next = kNativeThreads;
  }
  const bool has_flags = __syncthreads_or(flag_any) != 0;
  const int64_t nu = (int64_t)A.dup * nd;
  const int64_t ug0 = (int64_t)A.dup * (d0 - A.kp_off[0]);  // global index of the partition's unit 0
  const uint64_t key = part_key(A.native_seed, A.part_seed[p]);
  const int32_t max_num = A.seq - 3;
  int64_t r = threadIdx.x;
  bool fresh = true;
  CtrRng rng(key, 0, kStreamWalk);
  int32_t s0 = 0, ns = 0, i = 0, target = 0, dl = 0;
  int64_t np = 0, base = 0;
  while (__builtin_amdgcn_ballot_w64(r < nu)) {
    if (r < nu) {
      if (fresh) {  // a new unit: its document and target length (pretrain.py:259-262)
        fresh = false;
        dl = (int32_t)(r % nd);
        rng = CtrRng(key, r, kStreamWalk);
        s0 = W.doc(dl);
        ns = W.doc(dl + 1) - s0;
        i = 0;
        np = 0;
        if (EMIT) base = A.uoff[ug0 + r];
        target = max_num;
        if (rng.rand53() < A.k_short) target = (int32_t)rng.randint(2, max_num);
      }
      if (i < ns) {  // one chunk -> one pair
        const int64_t c_pre = W.pre(s0 + i);
        const int32_t e = first_reaching(W, s0 + i, s0 + ns, c_pre + target) - s0;
        const int32_t chunk0 = i, chunk_n = e - i + 1;
        const int32_t a_end = chunk_n >= 2 ? (int32_t)rng.randint(1, chunk_n - 1) : 1;
        const int64_t la = W.pre(s0 + chunk0 + a_end) - c_pre;
        int64_t lb, b_ks;
        int32_t rn = 0, flags = 0;
        if (chunk_n == 1 || rng.coin()) {  // random next (pretrain.py:291-321)
          rn = 1;
          const int64_t target_b = target - la;
          int64_t rd = 0;
          for (int t = 0; t < 10; ++t) {
            rd = rng.randint(0, nd - 1);
            if (rd != dl) break;
          }
          if (rd == dl) rn = 0;
          const int32_t r0 = W.doc(rd), rns = W.doc(rd + 1) - r0;
          const int32_t rstart = (int32_t)rng.randint(0, rns - 1);
          const int64_t b_pre = W.pre(r0 + rstart);
          const int32_t be = first_reaching(W, r0 + rstart, r0 + rns, b_pre + target_b);
          lb = W.pre(be + 1) - b_pre;
          b_ks = sb + r0 + rstart;
          if (EMIT && A.masking)
            flags = range_flags(A, has_flags, sb, s0 + chunk0, s0 + chunk0 + a_end) |
                    range_flags(A, has_flags, sb, r0 + rstart, be + 1);
          i = chunk0 + a_end;  // the unused segments are put back (pretrain.py:320-321)
        } else {
          lb = W.pre(s0 + e + 1) - W.pre(s0 + chunk0 + a_end);
          b_ks = sb + s0 + chunk0 + a_end;
          if (EMIT && A.masking) flags = range_flags(A, has_flags, sb, s0 + chunk0, s0 + e + 1);
          i = e + 1;
        }
        // _truncate_seq_pair: which side each trim hits is fixed (see WaveRng::trunc_draws); front
        // or back is a fair coin per trim
        int32_t na = (int32_t)la, nb = (int32_t)lb, a_front = 0, b_front = 0;
        const int32_t T = na + nb - max_num;
        if (T > 0) {
          const int32_t dd = na - nb, ad = dd < 0 ? -dd : dd;
          const int32_t nA = (dd > 0 ? min(dd, T) : 0) + (T > ad ? (T - ad) / 2 : 0);
          a_front = rng.heads(nA);
          b_front = rng.heads(T - nA);
          na -= nA;
          nb -= T - nA;
        }
        if (EMIT) {
          const int64_t q = base + np;
          const int64_t a_ks = sb + s0 + chunk0;
          A.desc[q] = PairDesc{a_ks, b_ks, a_front, na, b_front, nb | (int32_t)((uint32_t)rn << 31)};
          A.ppart[q] = (int32_t)p;
          if (A.masking) {
            int32_t nc = na + nb;
            if (flags) {  // literal [CLS]/[SEP] in the text are not candidates
              nc = 0;
              for (int32_t t = 0; t < na + nb; ++t) {
                const int32_t tok = t < na ? win_token(A, a_ks, a_front, t)
                                           : win_token(A, b_ks, b_front, t - na);
                nc += tok != A.cls_id && tok != A.sep_id;
              }
            }
            int32_t num = (int32_t)rint((double)(na + nb + 3) * A.ratio);
            if (num < 1) num = 1;
            if (num > nc) num = nc;
            A.nmask[q] = num;
            A.ncand[q] = nc;
          }
        }
        ++np;
      }
      if (i >= ns) {  // the unit is done: take the partition's next one
        if (!EMIT) A.ucnt[ug0 + r] = np;
        r = atomicAdd(&s_next, 1);
        fresh = true;
      }
    }
  }
}

// LDS words one partition's walk tables take; the largest over all partitions
__global__ void native_part_need_kernel(const int64_t* kp_off, const int64_t* kd_off, int64_t n_part,
                                        unsigned long long* need_max) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_part) return;
  const int64_t d0 = kp_off[p], d1 = kp_off[p + 1];
  atomicMax(need_max, (unsigned long long)(kd_off[d1] - kd_off[d0] + (d1 - d0) + 2));
}

struct KeptLenOnly {
  const int32_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i] & kLenMask; }
};

__global__ void native_part_base_kernel(const int64_t* kp_off, int64_t n_part, int32_t dup,
                                        const int64_t* uoff, int64_t* part_base) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n_part) part_base[p] = uoff[(int64_t)dup * (kp_off[p] - kp_off[0])];
}

// Uniform integer in [0, n) from a 32-bit draw: Lemire's multiply-shift with the exact rejection
// (taken with probability < n / 2^32, so the lanes of a wave stay in step).
__device__ inline uint32_t lemire_below(uint32_t x, uint32_t n, CtrRng& rng) {
  uint64_t m = (uint64_t)x * n;
  if ((uint32_t)m < n) {
    const uint32_t t = (0u - n) % n;
    while ((uint32_t)m < t) m = (uint64_t)rng.u32() * n;
  }
  return (uint32_t)(m >> 32);
}

// 80 / 10 / 10 of create_masked_lm_predictions (pretrain.py:214-229) on one 32-bit draw:
// [MASK] below ceil(0.8 * 2^32), the original token below ceil(0.9 * 2^32), else a random token.
constexpr uint32_t kNat80 = 3435973837u, kNat90 = 3865470567u;

// Masked positions of ppw consecutive pairs per wave (one lane per pair; 64, or fewer where the
// staged masks of 64 pairs exceed the LDS budget, the lanes above ppw idle), in lock step so that
// every lane's Philox refill comes at the same iteration:
//  1. Floyd's sampling of num candidate indices out of nc (a uniform num-subset: the shuffled
//     prefix of pretrain.py:197-207), one draw per step, into a lane-private LDS bitmap;
//  2. the set bits in ascending order (= sorted(masked_lms, key=index)), each with an 80/10/10
//     decision from its own stream (two draws per mask, whatever the decision), staged in LDS;
//  3. the wave's masks are one contiguous run of the pool (moff is the planner-order scan), copied
//     out with coalesced stores.
// Every draw's stream position depends on the pair alone (the sampling and the decisions use
// separate streams), so a pair's masks do not depend on the pairs that share its wave.
__global__ void __launch_bounds__(256) mask_native_kernel(NativeArgs A, int32_t stage_cap, int32_t ppw) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mn[];
  const int w = wave_id(), lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int64_t q0 = ((int64_t)blockIdx.x * nw + w) * ppw;
  if (q0 >= A.n_pairs) return;
  uint32_t* bm = reinterpret_cast<uint32_t*>(s_mn) + (size_t)w * A.words * 64 + lane;
  int32_t* stok = reinterpret_cast<int32_t*>(s_mn + (size_t)nw * A.words * 64 * 4) + (size_t)w * stage_cap;
  uint16_t* spos = reinterpret_cast<uint16_t*>(s_mn + (size_t)nw * A.words * 64 * 4 +
                                                (size_t)nw * stage_cap * 4) + (size_t)w * stage_cap;
  const int64_t q = q0 + lane;
  const bool valid = lane < ppw && q < A.n_pairs;
  const int64_t qv = valid ? q : q0;
  const int64_t qe = q0 + ppw < A.n_pairs ? q0 + ppw : A.n_pairs;
  const int64_t m0 = A.moff[q0];
  const int32_t mend = (int32_t)(A.moff[qe] - m0);
  const int32_t num = valid ? A.nmask[qv] : 0;
  const int32_t nc = A.ncand[qv];
  const int32_t mb = (int32_t)(A.moff[qv] - m0);
  const PairDesc d = A.desc[qv];
  const int32_t na = d.na, nb = d.nb_rn & 0x7FFFFFFF;
  const int64_t p = A.ppart[qv];
  const uint64_t key = part_key(A.native_seed, A.part_seed[p]);
  const int64_t idx = qv - A.part_base[p];
  for (int i = 0; i < A.words; ++i) bm[i * 64] = 0u;
  CtrRng rng(key, idx, kStreamMask);
  for (int32_t s = 0; __builtin_amdgcn_ballot_w64(s < num); ++s) {
    const uint32_t u = rng.u32();
    if (s < num) {
      const uint32_t j = (uint32_t)(nc - num + s);
      const uint32_t t = lemire_below(u, j + 1u, rng);
      const uint32_t wt = bm[(t >> 5) * 64];
      const uint32_t pick = (wt >> (t & 31)) & 1u ? j : t;
      bm[(pick >> 5) * 64] |= 1u << (pick & 31);
    }
  }
  CtrRng drng(key, idx, kStreamDecide);
  const bool fast = nc == na + nb;
  int32_t wi = 0, tcur = 0, ccur = 0;  // bitmap word; slow path: token / candidate cursor
  uint32_t bits = num > 0 ? bm[0] : 0u;
  for (int32_t m = 0; __builtin_amdgcn_ballot_w64(m < num); ++m) {
    const uint32_t x = drng.u32(), y = drng.u32();
    if (m < num) {
      while (bits == 0u) bits = bm[++wi * 64];
      const int32_t ci = wi * 32 + __ffs(bits) - 1;
      bits &= bits - 1u;
      int32_t t = ci;
      if (!fast) {  // walk to the ci-th non-[CLS]/[SEP] token
        while (true) {
          const int32_t tok = tcur < na ? win_token(A, d.a_ks, d.a_front, tcur)
                                        : win_token(A, d.b_ks, d.b_front, tcur - na);
          if (tok != A.cls_id && tok != A.sep_id) {
            if (ccur == ci) break;
            ++ccur;
          }
          ++tcur;
        }
        t = tcur++;
        ++ccur;
      }
      const int32_t tok = x < kNat80 ? A.mask_id
                          : x < kNat90 ? kKeep
                                       : (int32_t)lemire_below(y, (uint32_t)A.vocab_size, drng);
      spos[mb + m] = (uint16_t)(t < na ? t + 1 : t + 2);
      stok[mb + m] = tok;
    }
  }
  wave_sync();
  for (int32_t i = lane; i < mend; i += 64) {
    A.mpos[m0 + i] = spos[i];
    A.mtok[m0 + i] = stok[i];
  }
}

// ---------------------------------------------------------------------------------------------
// Whole-word static masking (lddl_pair_params::whole_word): Google BERT's
// create_masked_lm_predictions with do_whole_word_mask on the native streams. The reference has
// no such mode, so it exists with LDDL_RNG_NATIVE only.
// ---------------------------------------------------------------------------------------------
// streams of the whole-word path (CtrRng keeps 4 bits for the stream id)
enum : uint32_t { kStreamWordKey = 5, kStreamWordDecide = 6 };

// The draws that belong to token t of a pair: Philox blocks (t << 16) + 0, 1, .. of the pair's
// stream (t < 65536: check_plan_args bounds seq), so no two tokens share a block.
__device__ inline CtrRng token_rng(uint64_t key, int64_t pair_index, uint32_t stream, int32_t t) {
  CtrRng r(key, pair_index, stream);
  r.blk = (uint32_t)t << 16;
  return r;
}

// Minimum of v over the 64 lanes (all lanes active), wave-uniform: an inclusive min-scan with the
// DPP steps of wave_incl_scan (a lane without a source keeps its own value), read from lane 63.
template <int kCtrl, int kRowMask>
__device__ inline uint32_t min_step(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, kRowMask, 0xF, false);
  return o < v ? o : v;
}
__device__ inline uint32_t wave_min_u32(uint32_t v) {
  v = min_step<0x111, 0xF>(v);  // row_shr:1
  v = min_step<0x112, 0xF>(v);  // row_shr:2
  v = min_step<0x114, 0xF>(v);  // row_shr:4
  v = min_step<0x118, 0xF>(v);  // row_shr:8
  v = min_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v = min_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// smallest entry of the lane's column (tokens wi * 64 + lane) among the windows in `cand`
__device__ inline uint64_t column_min(const uint64_t* kk, uint64_t cand, int lane) {
  uint64_t best = ~0ull;
  for (uint64_t c = cand; c; c &= c - 1) {
    const uint64_t v = kk[(__ffsll((unsigned long long)c) - 1) * 64 + lane];
    best = v < best ? v : best;
  }
  return best;
}

// One wave per pair, lane = token of a 64-token window. The budget is the plain path's num
// (nmask[q], from plan_native_kernel<true>); the pool is laid out by it (moff) and the number of
// positions actually masked is written back to nmask[q] (<= the budget, possibly 0), which is what
// pair_prep_kernel and the gather then read.
//  1. tokens loaded coalesced; per window the ballots of literal [CLS]/[SEP] and of word starts
//     (a token that is no continuation; tokens past the pair count as starts), the special flag
//     of a window's last token carried into the next; one Philox key per head, entry
//     key << 32 | token << 16 | word length in the lane's LDS column;
//  2. the greedy walk of the shuffled word order as a repeated wave-wide select-min over the
//     entries not yet visited: every lane keeps its column's smallest entry, a 32-bit DPP minimum
//     of the keys and a ballot name the winner, i.e. the words come in (key, lane, window) order
//     (two of W words share a key in W^2 / 2^33 of the pairs, 1e-5 at seq 512); a word is taken
//     iff it still fits; only the winner's lane rescans its column;
//  3. lane w holds the masked bits of window w: ranks by popcount, sorted positions, and an
//     80/10/10 decision per masked token from the token's own Philox block.
// Every cross-lane step (ballots, DPP minimum) is reached by all 64 lanes: the loops run on
// wave-uniform bounds and tails are predicated.
__global__ void __launch_bounds__(256) mask_ww_native_kernel(NativeArgs A, ContBits C, int32_t seqp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_ww[];
  const int w = wave_id(), lane = threadIdx.x & 63, nwv = blockDim.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * nwv + w;
  if (q >= A.n_pairs) return;
  const int32_t wcap = seqp >> 6;  // windows of the longest pair
  uint64_t* kk = reinterpret_cast<uint64_t*>(s_ww) + (size_t)w * (seqp + wcap + 1);  // [seqp]
  uint64_t* sbits = kk + seqp;  // [wcap + 1] word-start ballots, then the masked bits, per window
  const PairDesc d = A.desc[q];
  const int32_t na = __builtin_amdgcn_readfirstlane(d.na);
  const int32_t n = __builtin_amdgcn_readfirstlane(min(d.na + (d.nb_rn & 0x7FFFFFFF), seqp));
  const int32_t nwin = (n + 63) >> 6;
  const int32_t budget = __builtin_amdgcn_readfirstlane(A.nmask[q]);
  const int64_t p = A.ppart[q];
  const uint64_t key = part_key(A.native_seed, A.part_seed[p]);
  const int64_t idx = q - A.part_base[p];
  const int64_t a0 = A.kscan[d.a_ks] + d.a_front, b0 = A.kscan[d.b_ks] + d.b_front - na;
  bool carry = false;   // the token before the window is a literal special
  uint64_t cand = 0;    // bit wi: token wi * 64 + lane is a head not yet visited
  for (int32_t wi = 0; wi < nwin; ++wi) {
    const int32_t t = wi * 64 + lane;
    const bool in = t < n;
    const int32_t id = in ? A.dense.ld((t < na ? a0 : b0) + t) : 0;
    const bool special = in && (id == A.cls_id || id == A.sep_id);
    const uint64_t sp = ballot(special);
    const bool prev_special = lane ? ((sp >> (lane - 1)) & 1) != 0 : carry;
    carry = (sp >> 63) != 0;
    const bool cont = in && !special && t != 0 && t != na && !prev_special && cont_id(C, id);
    const uint64_t st = ballot(!cont);
    if (lane == 0) sbits[wi] = st;
    if (in && !special && !cont) {
      CtrRng r = token_rng(key, idx, kStreamWordKey, t);
      kk[t] = ((uint64_t)r.u32() << 32) | ((uint64_t)t << 16);
      cand |= 1ull << wi;
    }
  }
  if (lane == 0) sbits[nwin] = ~0ull;  // (a pair that fills its last window: the word ends there)
  wave_sync();
  // word lengths: the distance to the next start
  for (uint64_t c = cand; c; c &= c - 1) {
    const int32_t wi = __ffsll((unsigned long long)c) - 1;
    uint64_t m = lane < 63 ? sbits[wi] >> (lane + 1) : 0ull;
    int32_t len = __ffsll((unsigned long long)m);
    if (!m) {
      int32_t w2 = wi + 1;
      while (!(m = sbits[w2])) ++w2;  // (ends at sbits[nwin] at the latest)
      len = 64 - lane + 64 * (w2 - wi - 1) + __ffsll((unsigned long long)m) - 1;
    }
    kk[wi * 64 + lane] |= (uint64_t)(uint32_t)len;
  }
  uint64_t best = column_min(kk, cand, lane);
  uint64_t mb = 0;  // lane wi: masked tokens of window wi
  int32_t masked = 0;
  while (masked < budget) {
    // the smallest key; among the lanes that hold it (nearly always one) the lowest wins
    const uint32_t kmin = wave_min_u32((uint32_t)(best >> 32));
    const uint64_t win = ballot(cand != 0 && (uint32_t)(best >> 32) == kmin);
    if (!win) break;  // every word visited
    const int wl = __ffsll((unsigned long long)win) - 1;
    const uint32_t sel = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)best, wl);
    const int32_t h = (int32_t)(sel >> 16), len = (int32_t)(sel & 0xFFFF);
    if (masked + len <= budget) {
      masked += len;
      const int32_t lo = max(h - 64 * lane, 0), hi = min(h + len - 64 * lane, 64);
      if (lo < hi) mb |= (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1) << lo;
    }
    if (lane == wl) {
      cand &= ~(1ull << (h >> 6));
      best = column_min(kk, cand, lane);
    }
  }
  wave_sync();  // (the start ballots are read; their slots take the masked bits)
  if (lane < nwin) sbits[lane] = mb;
  wave_sync();
  const int64_t m0 = A.moff[q];
  int32_t base = 0;
  for (int32_t wi = 0; wi < nwin; ++wi) {
    const uint64_t m = sbits[wi];
    if ((m >> lane) & 1) {
      const int32_t t = wi * 64 + lane;
      const int64_t at = m0 + base + (int32_t)popc_below(m);
      CtrRng drng = token_rng(key, idx, kStreamWordDecide, t);
      const uint32_t x = drng.u32(), y = drng.u32();
      A.mpos[at] = (uint16_t)(t < na ? t + 1 : t + 2);
      A.mtok[at] = x < kNat80 ? A.mask_id
                   : x < kNat90 ? kKeep
                                : (int32_t)lemire_below(y, (uint32_t)A.vocab_size, drng);
    }
    base += __popcll(m);
  }
  if (lane == 0) A.nmask[q] = base;
}

// random.shuffle(partition_pairs), native: output row k of partition p takes pair perm_p(k), a
// keyed 4-round Feistel bijection on [0, 4^h) >= np restricted to [0, np) by cycle walking.
__global__ void __launch_bounds__(256) order_native_kernel(NativeArgs A) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= A.n_pairs) return;
  const int64_t p = A.ppart[q];
  const int64_t pb = A.part_base[p], np = A.part_base[p + 1] - pb;
  const uint64_t key = mix64(part_key(A.native_seed, A.part_seed[p]) ^ kStreamOrder);
  int bits = 1;
  while ((1ll << bits) < np) ++bits;
  const int h = (bits + 1) >> 1;
  const uint64_t hm = (1ull << h) - 1;
  uint64_t x = (uint64_t)(q - pb);
  do {
    uint64_t L = x >> h, R = x & hm;
    for (uint64_t rd = 0; rd < 4; ++rd) {
      const uint64_t f = mix64(R ^ key ^ (rd << 56)) & hm;
      const uint64_t nl = R;
      R = L ^ f;
      L = nl;
    }
    x = (L << h) | R;
  } while (x >= (uint64_t)np);
  A.src[q] = pb + (int64_t)x;
}

}  // namespace

// LDDL_RNG_NATIVE control plane: count pass, unit scan, emit pass, mask offsets + masks, order,
// layout.
int plan_native(lddl_pairs* P, PlanWork& W) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = W.n_part;
  hipStream_t st = W.st;
  NativeArgs A{};
  fill_plan_args(A, P, W);
  int64_t kp_ends[2] = {0, 0};  // kept documents covered by the partitions
  unsigned long long need_max = 0, *d_need;
  int rc;
  if ((rc = W.tmp.take(&d_need, 1))) return rc;
  LDDL_HIP(hipMemsetAsync(d_need, 0, 8, st));
  if (n_part)
    hipLaunchKernelGGL(native_part_need_kernel, dim3((unsigned)((n_part + 255) / 256)), dim3(256), 0, st,
                       P->kp_off, P->kd_off, n_part, d_need);
  LDDL_HIP(hipMemcpyAsync(&kp_ends[0], P->kp_off, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&kp_ends[1], P->kp_off + n_part, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(&need_max, d_need, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  A.unit0 = (int64_t)prm->dup * kp_ends[0];
  A.n_units = (int64_t)prm->dup * (kp_ends[1] - kp_ends[0]);
  A.native_seed = prm->native_seed;
  const int64_t nu = A.n_units;
  // walk tables in LDS up to 96 KB per workgroup; larger partitions read a global prefix
  int64_t kLdsWordsCap = 24576;
  if (const char* e = getenv("LDDL_NATIVE_LDS_WORDS")) kLdsWordsCap = atoll(e);  // tests: global path
  const int32_t lds_words = (int32_t)std::max<int64_t>(
      1, std::min<int64_t>((int64_t)need_max, kLdsWordsCap));
  int64_t *uoff, *scr, *g_pre = nullptr;
  if ((rc = W.tmp.take(&A.ucnt, nu)) || (rc = W.tmp.take(&uoff, nu + 1)) ||
      (rc = W.tmp.take(&scr, scan_scratch_elems(std::max(nu, P->n_kept_sent) + 1))))
    return rc;
  if ((int64_t)need_max > kLdsWordsCap) {
    if ((rc = W.tmp.take(&g_pre, P->n_kept_sent + 1))) return rc;
    LDDL_HIP(scan_exclusive(KeptLenOnly{P->ks_len}, P->n_kept_sent, g_pre, scr, st));
  }
  LDDL_HIP(hipEventRecord(P->ev[0], st));
  const size_t lds_bytes = (size_t)4 * lds_words;
  if (n_part && nu)
    hipLaunchKernelGGL(plan_native_kernel<false>, dim3((unsigned)n_part), dim3(kNativeThreads), lds_bytes,
                       st, A, g_pre, lds_words);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(scan_i64(A.ucnt, nu, uoff, scr, st));
  LDDL_HIP(hipMemcpyAsync(&P->n_pairs, uoff + nu, 8, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  const int64_t n = P->n_pairs;
  A.uoff = uoff;
  A.n_pairs = n;
  if ((rc = P->mem.take(&P->part_base, n_part + 1)) || (rc = P->mem.take(&P->desc, n)) ||
      (rc = W.tmp.take(&A.ppart, n)) || (rc = P->mem.take(&P->src, n)))
    return rc;
  if (prm->masking &&
      ((rc = P->mem.take(&P->nmask, n)) || (rc = W.tmp.take(&A.ncand, n)) ||
       (rc = P->mem.take(&P->moff, n + 1)) || (rc = W.tmp.take(&scr, scan_scratch_elems(n + 1)))))
    return rc;
  hipLaunchKernelGGL(native_part_base_kernel, dim3((unsigned)((n_part + 256) / 256)), dim3(256), 0,
                     st, P->kp_off, n_part, prm->dup, uoff, P->part_base);
  A.part_base = P->part_base;
  A.desc = P->desc;
  A.nmask = P->nmask;
  if (n_part && nu)
    hipLaunchKernelGGL(plan_native_kernel<true>, dim3((unsigned)n_part), dim3(kNativeThreads), lds_bytes,
                       st, A, g_pre, lds_words);
  LDDL_HIP(hipGetLastError());
  const unsigned gp = (unsigned)((n + 255) / 256);
  if (prm->masking) {
    LDDL_HIP(scan_exclusive(I32{P->nmask}, n, P->moff, scr, st));
    LDDL_HIP(hipMemcpyAsync(&P->n_masked, P->moff + n, 8, hipMemcpyDeviceToHost, st));
    LDDL_HIP(hipStreamSynchronize(st));
    if ((rc = P->mem.take(&P->mpos, P->n_masked)) || (rc = P->mem.take(&P->mtok, P->n_masked)))
      return rc;
    A.moff = P->moff;
    A.mpos = P->mpos;
    A.mtok = P->mtok;
    A.words = (prm->seq + 31) / 32;
    // per wave: the 64 lanes' bitmaps + the staged masks of its ppw pairs (<= max_pred each);
    // up to 4 waves per workgroup within 64 KB of LDS. 64 pairs per wave while their staging fits
    // that budget, else half as many until it does (seq 4096 at ratio 0.15: 8; one pair of 4096
    // masks, ratio 1.0, takes 56 KB). Sized for 64 pairs whatever the ratio, seq 512 at ratio 1.0
    // (196 KB) or seq 2500 at 0.15 would ask for more LDS than a CU has
    const int32_t mp = std::max(P->max_pred, 1);
    auto wave_bytes = [&](int32_t pairs) { return (size_t)A.words * 64 * 4 + (size_t)pairs * mp * 6; };
    int32_t ppw = 64;
    while (ppw > 1 && wave_bytes(ppw) > 65536) ppw >>= 1;
    const int32_t stage_cap = ppw * mp;
    const size_t per_wave = wave_bytes(ppw);
    const int nwv = (int)std::max<size_t>(1, std::min<size_t>(4, 65536 / per_wave));
    const int64_t per_wg = (int64_t)ppw * nwv;  // pairs per workgroup
    if (n && !prm->whole_word)
      hipLaunchKernelGGL(mask_native_kernel, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(64 * nwv),
                         per_wave * nwv, st, A, stage_cap, ppw);
    if (n && prm->whole_word) {
      // one wave per pair; per wave an 8-byte entry per token of the longest pair (seq - 3,
      // rounded up to whole windows) and a ballot per window + 1; up to 4 waves within 64 KB
      const int32_t seqp = (prm->seq - 3 + 63) / 64 * 64;
      const size_t ww_wave = (size_t)8 * (seqp + seqp / 64 + 1);
      const int wwv = (int)std::max<size_t>(1, std::min<size_t>(4, 65536 / ww_wave));
      hipLaunchKernelGGL(mask_ww_native_kernel, dim3((unsigned)((n + wwv - 1) / wwv)), dim3(64 * wwv),
                         ww_wave * wwv, st, A, ContBits{W.c->d_cont_bits, W.c->vocab_size}, seqp);
    }
    LDDL_HIP(hipGetLastError());
  }
  A.src = P->src;
  if (n) hipLaunchKernelGGL(order_native_kernel, dim3(gp), dim3(256), 0, st, A);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipEventRecord(P->ev[1], st));
  return layout_pairs(P, W);
}

}  // namespace lddl
