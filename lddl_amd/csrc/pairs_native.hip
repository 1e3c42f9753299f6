// Pair stage, the native planner (LDDL_RNG_NATIVE): the reference's algorithms on counter-based
// Philox streams (native_dev.h): the walk planner, the keyed partition order and the control
// plane, plan_native. Its mask kernels are a unit of their own (pairs_native_mask.hip), and the
// shapes of the dynamic-LDS launches come from native_shape.h.
#include "native_dev.h"
#include "native_shape.h"

// (scan functor over the masks per pair; at file scope, where it has always been: the scan
// kernels instantiated over it keep their names)
struct I32 {
  const int32_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i]; }
};

namespace lddl {
namespace {

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
  // walk tables in LDS up to the cap; larger partitions read a global prefix
  // (LDDL_NATIVE_LDS_WORDS, tests: a small cap, so that the global path runs)
  const WalkLds walk =
      native_walk_lds(need_max, W.knobs.native_lds_words >= 0 ? W.knobs.native_lds_words : kNativeLdsWordsCap);
  int64_t *uoff, *scr, *g_pre = nullptr;
  if ((rc = W.tmp.take(&A.ucnt, nu)) || (rc = W.tmp.take(&uoff, nu + 1)) ||
      (rc = W.tmp.take(&scr, scan_scratch_elems(std::max(nu, P->n_kept_sent) + 1))))
    return rc;
  if (walk.global_prefix) {
    if ((rc = W.tmp.take(&g_pre, P->n_kept_sent + 1))) return rc;
    LDDL_HIP(scan_exclusive(KeptLenOnly{P->ks_len}, P->n_kept_sent, g_pre, scr, st));
  }
  LDDL_HIP(hipEventRecord(P->ev[0], st));
  if (n_part && nu)
    hipLaunchKernelGGL(plan_native_kernel<false>, dim3((unsigned)n_part), dim3(kNativeThreads), walk.bytes(),
                       st, A, g_pre, walk.words);
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
    hipLaunchKernelGGL(plan_native_kernel<true>, dim3((unsigned)n_part), dim3(kNativeThreads), walk.bytes(),
                       st, A, g_pre, walk.words);
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
    launch_native_masks(P, W, A);
    LDDL_HIP(hipGetLastError());
  }
  A.src = P->src;
  if (n) hipLaunchKernelGGL(order_native_kernel, dim3(gp), dim3(256), 0, st, A);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipEventRecord(P->ev[1], st));
  return layout_pairs(P, W);
}

}  // namespace lddl
