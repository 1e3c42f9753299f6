// Pair stage, the replay planner (LDDL_RNG_REPLAY; the stage's other units and its orchestration:
// file map in pairs_api.hip): plan_replay_kernel, the three one-purpose kernels beside it and the
// host side of one-range, sliced and split plans (lddl/dask/bert/pretrain.py:161-176, 182-238,
// 241-365, 386-402). The kernel's device pieces are headers: CPython's MT19937 wave-uniform
// (replay_rng.h), the sentence-length window (replay_len.h), the time-sliced queue
// (replay_slice.h) and one wave's share of the dense packing (densify_dev.h).
#include <cstdio>
#include <type_traits>
#include <vector>

#include "densify_dev.h"
#include "pairs_plan.h"
#include "replay_len.h"
#include "replay_rng.h"
#include "replay_slice.h"

namespace lddl {
namespace {

constexpr int64_t kPoolChunk = 4096;  // mask pool entries reserved per atomic
constexpr uint64_t kLt08 = 7205759403792794ull;  // ceil(0.8 (binary64) * 2^53): random() < 0.8

// waves per SIMD the compiler must keep: 8 caps the kernel at 78 SGPRs (140 spilled to VGPR
// lanes); 6 lets it use all 106 (59 spilled) at 7 waves/SIMD, 176 -> 169.6 ms per 10 GB
// (profiles/r02_plan_minw_ab.txt)
// kDocsLds: every partition's document offsets fit the LDS table (host-checked: <= kDocLds
// documents), so the document lookups carry no global-memory branch; kJB: bytes per shuffle draw;
// kSliced: the time-sliced mode (replay_slice.h)
template <bool kDocsLds, int kJB, bool kSliced = false>
__global__ void __launch_bounds__(64, 6) plan_replay_kernel(PlanArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint32_t* s_mt = reinterpret_cast<uint32_t*>(smem);
  int32_t* s_doc = reinterpret_cast<int32_t*>(s_mt + kN + kLook);  // [kDocLds + 1]
  const int lane = threadIdx.x;
  const bool leader = lane == 0;
  if (!kSliced && (int)blockIdx.x >= A.n_part) {
    // Workgroups past the partitions pack `dense` (what densify_kernel would do after this
    // launch). Dispatched in order, they start as the last partitions' waves are placed and
    // run in the slots the planner's tail leaves idle (a separate launch before or beside the
    // planner delays its dispatch).
    const int64_t k_lo = A.dense_lo ? *A.dense_lo : 0;
    for (int64_t g = (int)blockIdx.x - A.n_part; k_lo + g * 64 < A.n_kept_sent; g += A.n_dense_wg)
      densify_group(k_lo + g * 64, A.ks_start, A.ks_len, A.kscan, A.n_kept_sent, A.ids, A.dense);
    return;
  }
  // sliced: the wave's current ticket and whether the partition is taken up from its save area
  [[maybe_unused]] int32_t ticket = 0;
  [[maybe_unused]] bool parked = false;
  int p = A.p0 + (int)blockIdx.x;
  if constexpr (kSliced) {
    ticket = slice_claim(A, &p);
    parked = ticket >= A.n_part;
  }
  if (!kSliced || ticket >= 0) do {  // (sliced: one slice per turn; else the body runs once)
#ifdef LDDL_STAMPS
  uint64_t st_acc[kStampRegions] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  [[maybe_unused]] uint64_t st_t = STAMP_T();
#ifdef LDDL_STAMPS
  const uint64_t rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  WaveRng rng{s_mt, 0, 0, 0, 0u
#ifdef LDDL_STAMPS
              , 0, 0
#endif
  };
  // this wave's current chunks of the mask pool and of the shuffle-draw pool: next entry, entries
  // left (32-bit compares), and whether the chunk lies inside the pool
  int64_t pool_cur = 0, jpool_cur = 0;
  int32_t pool_left = 0, jpool_left = 0;
  bool pool_fits = true, jpool_fits = true;
  int64_t np = 0;
  // sliced: where the slice starts (dp0, di0), and the documents left in it
  [[maybe_unused]] int dp0 = 0;
  [[maybe_unused]] int32_t di0 = 0, slice_left = 0;
  [[maybe_unused]] bool yielded = false;
  if (kSliced && parked) {
    // the one acquire of the hand-off, then the state by vector loads (lane-indexed addresses)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    uint64_t* sv = A.sl_save + (int64_t)p * kSaveU64;
    uint64_t* s64 = reinterpret_cast<uint64_t*>(s_mt);
    for (int i = lane; i < kSaveU64; i += 64) s64[i] = sv[i];
    __syncthreads();
    const int32_t* h = s_doc;  // the header words (ParkWord) follow the MT block
    rng.mti = uni(h[kParkMti]);
    dp0 = uni(h[kParkDp]);
    di0 = uni(h[kParkDi]);
    np = ((int64_t)uni(h[kParkNpHi]) << 32) | (uint32_t)uni(h[kParkNpLo]);
    pool_cur = ((int64_t)uni(h[kParkPoolHi]) << 32) | (uint32_t)uni(h[kParkPoolLo]);
    pool_left = uni(h[kParkPoolLeft]);
    jpool_cur = ((int64_t)uni(h[kParkJpoolHi]) << 32) | (uint32_t)uni(h[kParkJpoolLo]);
    jpool_left = uni(h[kParkJpoolLeft]);
    const int32_t fb = uni(h[kParkFits]);
    pool_fits = (fb & 1) != 0;
    jpool_fits = (fb & 2) != 0;
    __syncthreads();  // (before the document table overwrites the header)
  } else {
    rng.seed_i64(A.part_seed[p]);
  }
  const int64_t d0 = A.kp_off[p];
  const int32_t nd = (int32_t)(A.kp_off[p + 1] - d0);  // (partition-local indices are 32-bit)
  const int64_t kbase = A.kd_off[d0];
  if (kDocsLds)
    for (int64_t d = lane; d <= nd; d += 64) s_doc[d] = (int32_t)(A.kd_off[d0 + d] - kbase);
  __syncthreads();
  auto doc_loc = [&](int32_t d) -> int32_t {  // first kept sentence of document d, partition-local
    if constexpr (kDocsLds) return uni(s_doc[d]);
    else return uni((int32_t)(A.kd_off[d0 + d] - kbase));
  };
  const int32_t* ks_len_p = A.ks_len + kbase;
  const int64_t base = (int64_t)A.dup * kbase;
  const int32_t max_num = A.seq - 3;
  LenWin La, Lb;
  constexpr int kPrioLevels = 4;  // priority levels used (s_setprio has 4)
  // issue priority by progress: a SIMD issues its highest-priority (then oldest) wave first, so
  // waves that are behind (e.g. a partition dispatched into a freed slot) catch up and the waves
  // of a SIMD finish together instead of leaving the last ones running alone
  int prio_q = -1;
  const int64_t prio_tot = (int64_t)A.dup * nd;
  // the priority steps at the document counts where progress crosses a quarter (no 64-bit
  // division per document)
  int32_t prio_next = 0, prio_done = 0;
  if constexpr (kSliced) {  // the slice's quantum (plan_slice_quantum, per partition)
    const int64_t q = A.sl_quantum ? (int64_t)A.sl_quantum
                                   : (prio_tot + kPlanSliceK - 1) / kPlanSliceK;
    slice_left = (int32_t)std::min<int64_t>(std::max<int64_t>(q, 1), INT32_MAX);
  }
  if (nd > 0) La.prefetch(ks_len_p + doc_loc(di0), doc_loc(di0 + 1) - doc_loc(di0));
  for (int dp = dp0; dp < A.dup; ++dp) {
    for (int32_t di = di0; di < nd; ++di) {
      if constexpr (kSliced) {
        if (slice_left == 0) {
          // The quantum is used up and document (dp, di) is still to plan: park the partition.
          // The header words go behind the MT block in LDS (over the document table, which the
          // next slice loads again), then the block leaves as 8-byte write-through stores.
          int32_t hw = 0;
          int32_t hv[kParkWords];
          hv[kParkMti] = rng.mti;
          hv[kParkDp] = dp;
          hv[kParkDi] = di;
          hv[kParkNpLo] = (int32_t)np;
          hv[kParkPoolLo] = (int32_t)pool_cur;
          hv[kParkPoolHi] = (int32_t)(pool_cur >> 32);
          hv[kParkPoolLeft] = pool_left;
          hv[kParkJpoolLo] = (int32_t)jpool_cur;
          hv[kParkJpoolHi] = (int32_t)(jpool_cur >> 32);
          hv[kParkJpoolLeft] = jpool_left;
          hv[kParkFits] = (pool_fits ? 1 : 0) | (jpool_fits ? 2 : 0);
          hv[kParkNpHi] = (int32_t)(np >> 32);
#pragma unroll
          for (int k = 0; k < kParkWords; ++k)
            if (lane == k) hw = hv[k];
          __syncthreads();
          if (lane < kSaveHdr) s_doc[lane] = hw;
          __syncthreads();
          uint64_t* sv = A.sl_save + (int64_t)p * kSaveU64;
          const uint64_t* s64 = reinterpret_cast<const uint64_t*>(s_mt);
          for (int i = lane; i < kSaveU64; i += 64) __hip_atomic_store(sv + i, s64[i], LDDL_RLX_AGENT);
          __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drained before the publish
          yielded = true;
          break;
        }
        --slice_left;
      }
      if (!kSliced && prio_done >= prio_next) {
        ++prio_q;
        prio_next = (int32_t)(((int64_t)(prio_q + 1) * prio_tot + kPrioLevels - 1) / kPrioLevels);
        const int lvl = kPrioLevels - 1 - prio_q;
        if (lvl >= 3) __builtin_amdgcn_s_setprio(3);
        else if (lvl == 2) __builtin_amdgcn_s_setprio(2);
        else if (lvl == 1) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
      }
      ++prio_done;
      const int32_t ls0 = doc_loc(di);
      const int64_t s0 = kbase + ls0;
      const int ns = doc_loc(di + 1) - ls0;
      // (the document's first length window was loaded one document ago; 1.5 ms per 10 GB,
      // profiles/r06p2_planner_loop_ab.txt)
      La.reset_prefetched(ks_len_p + ls0, ns);
      {
        const int32_t dn = di + 1 < nd ? di + 1 : 0;  // the next document (of this or the next pass)
        const int32_t nl0 = doc_loc(dn);
        La.prefetch(ks_len_p + nl0, doc_loc(dn + 1) - nl0);
      }
      int32_t target = max_num;
      if (rng.rand53() < A.k_short) target = rng.randint32(2, max_num);
      // chunks: sentences are accumulated until the target length or the document end
      // (pretrain.py:276-280); after a random-next pair the unused sentences are put back
      // (320-321), so the next chunk starts right after A
      for (int chunk0 = 0; chunk0 < ns;) {
        const int i = La.find(chunk0, ns, target);  // the chunk is [chunk0, i]
        const int chunk_n = i - chunk0 + 1;
        const int a_end = chunk_n >= 2 ? rng.randint32(1, chunk_n - 1) : 1;
        int32_t flags = 0;
        const int64_t la = La.sum(chunk0, chunk0 + a_end, flags);
        int64_t lb = 0, b_ks;
        int32_t rn = 0;
        int next0;
        STAMP_ADD(0, st_t);
        if (chunk_n == 1 || rng.below_half()) {
          rn = 1;
          const int64_t target_b = target - la;
          int32_t rd = 0;
          for (int t = 0; t < 10; ++t) {
            rd = rng.randint32(0, nd - 1);
            if (rd != di) break;
          }
          if (rd == di) rn = 0;
          const int32_t r0l = doc_loc(rd);
          const int rns = doc_loc(rd + 1) - r0l;
          const int rstart = rng.randint32(0, rns - 1);
          b_ks = kbase + (r0l + rstart);
          Lb.reset(ks_len_p + r0l, rns);
          const int jb = Lb.find(rstart, rns, target_b);  // B is [rstart, jb] (314-317)
          lb = Lb.sum(rstart, jb + 1, flags);
          next0 = chunk0 + a_end;
        } else {
          b_ks = s0 + chunk0 + a_end;
          lb = La.sum(chunk0 + a_end, i + 1, flags);
          next0 = i + 1;
        }
        STAMP_ADD(3, st_t);
        // _truncate_seq_pair
        int32_t a_front = 0, b_front = 0, na = (int32_t)la, nb = (int32_t)lb;
        rng.trunc_draws(na, nb, max_num, a_front, b_front);
        STAMP_ADD(5, st_t);
        const int64_t slot = base + np;
        // every lane stores the same record: the wave's identical writes merge into one, and no
        // exec-mask branch (3 scalar instructions + a branch) is spent on a leader-only store
        A.desc[slot] = PairDesc{s0 + chunk0, b_ks, a_front, na, b_front,
                                nb | (int32_t)((uint32_t)rn << 31)};
        if (A.masking) {
          // candidates = positions of [CLS] A [SEP] B [SEP] whose token is not [CLS]/[SEP]; only
          // their count matters here (fy_resolve_kernel recovers the positions)
          int32_t nc = na + nb;
          if (flags & kLenHasClsSep) {  // literal [CLS]/[SEP] inside A or B: inspect the tokens
            int32_t c = 0;
            for (int32_t t = 0; t < na + nb; ++t) {
              const int32_t tok = uni(t < na ? span_token(A, s0 + chunk0, a_front + t)
                                             : span_token(A, b_ks, b_front + (t - na)));
              c += tok != A.cls_id && tok != A.sep_id;
            }
            nc = uni(c);
          }
          STAMP_ADD(1, st_t);
          // num_to_predict = round(len(tokens) * masked_lm_ratio) (pretrain.py:197): binary64
          // product, round half to even - the IEEE operations Python performs
          int32_t num = uni((int32_t)__builtin_rint((double)(na + nb + 3) * A.ratio));
          if (num < 1) num = 1;
          if (num > nc) num = nc;
          // pool space for this pair's shuffle draws (nc) and masks (num): bump allocation in
          // per-wave chunks (one atomic per kPoolChunk entries); each slot records its offsets
          if (num > pool_left) {
            const int32_t sz = num > kPoolChunk ? (num + 7) & ~7 : (int32_t)kPoolChunk;
            int64_t nb0 = 0;
            if (leader) nb0 = (int64_t)atomicAdd(&A.pool_used[0], (unsigned long long)sz);
            nb0 = ((int64_t)uni((int)(nb0 >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)nb0);  // lane 0's
            pool_cur = nb0;
            pool_left = sz;
            pool_fits = nb0 + sz <= A.pool_cap;
          }
          if (nc > jpool_left) {
            const int32_t sz = nc > kPoolChunk ? (nc + 15) & ~15 : (int32_t)kPoolChunk;
            int64_t nb0 = 0;
            if (leader) nb0 = (int64_t)atomicAdd(&A.pool_used[2], (unsigned long long)sz);
            nb0 = ((int64_t)uni((int)(nb0 >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)nb0);
            jpool_cur = nb0;
            jpool_left = sz;
            jpool_fits = nb0 + sz <= A.jpool_cap;
          }
          const int64_t mb = pool_cur, jb = jpool_cur;
          // 16-byte aligned regions (fy_resolve_kernel's uint4 I/O; 1-byte draws too); chunk sizes
          // are multiples of the steps, so num <= left implies step <= left
          pool_cur += (num + 7) & ~7;
          pool_left -= (num + 7) & ~7;
          jpool_cur += (nc + 15) & ~15;
          jpool_left -= (nc + 15) & ~15;
          const bool fits = pool_fits && jpool_fits;
          if (!fits) *A.overflow = 1;  // (uniform; every lane stores the same flag)
          // random.shuffle(cand_indexes): draws j_i (i = nc-1 .. 1) to the pool
          // The region's tail [nc, nc rounded up to 16) gets j_i = i: fy_resolve's steps there move
          // an entry onto itself, so its step loop needs no per-step guard. (Entry 0 is not
          // written here: fy_draws' lanes store their rejected words there, and fy_resolve
          // takes j_0 = 0 itself.)
          const int32_t ip = nc + lane;
          {
            using Draw = std::conditional_t<kJB == 1, uint8_t, uint16_t>;
            Draw* jd = static_cast<Draw*>(A.jpool) + jb;
            rng.fy_draws(nc, [&](int32_t i, uint32_t j) {
              if (fits) jd[i] = (Draw)j;  // (fits is uniform: a scalar branch)
            });
            if (fits && ip < ((nc + 15) & ~15)) jd[ip] = (Draw)ip;
          }
          STAMP_ADD(2, st_t);
          // decisions of the masked candidates in shuffled order (pretrain.py:208-221)
          for (int32_t c0 = 0; c0 < num; c0 += 64) {
            const int cmax = min(64, num - c0);
            const int32_t mytok = rng.mask_decisions(cmax, kLt08, A.vocab_size, A.mask_id);
            if (fits && lane < cmax) A.mtok[mb + c0 + lane] = mytok;
          }
          STAMP_ADD(4, st_t);
          // (all lanes, as the descriptor above)
          A.spool[slot] = SlotPool{(uint32_t)(mb >> 3), (uint32_t)(jb >> 4), num, nc};
        }
        ++np;
        chunk0 = next0;
      }
    }
    if constexpr (kSliced) {
      if (yielded) break;
      di0 = 0;  // (the later passes start at the partition's first document)
    }
  }
  if (!kSliced || !yielded) {
  // random.shuffle(partition_pairs) (pretrain.py:401): record the draws j_i, i = np-1 .. 1
  // (64 at a time through writelane); shuffle_sort_kernel resolves the swaps.
  STAMP_ADD(0, st_t);
  {
    int32_t* js = A.jseq + base;
    rng.fy_draws(np, [&](int32_t i, uint32_t j) { js[i] = (int32_t)j; });  // (js[0] is never read)
  }
  STAMP_ADD(6, st_t);
  }
#ifdef LDDL_STAMPS
  if constexpr (kSliced) {  // the slices' regions add up per partition; the timeline is per ticket
    if (leader && A.stamps)
      for (int r = 0; r < kStampRegions - 1; ++r)
        atomicAdd(reinterpret_cast<unsigned long long*>(A.stamps) + (int64_t)p * kStampRegions + r,
                  (unsigned long long)st_acc[r]);
    if (leader && A.tl && !parked) A.tl[2 * (int64_t)p] = rt0;
    if (leader && A.tl && !yielded) A.tl[2 * (int64_t)p + 1] = __builtin_amdgcn_s_memrealtime();
    if (leader && A.tls && ticket >= 0) {
      A.tls[2 * (int64_t)ticket] = rt0;
      A.tls[2 * (int64_t)ticket + 1] = __builtin_amdgcn_s_memrealtime();
    }
  } else {
  st_acc[7] = rng.n_pass * 1000000 / (rng.n_win ? rng.n_win : 1);  // passes per window x 1e6
  if (leader && A.stamps)
    for (int r = 0; r < kStampRegions; ++r) A.stamps[(int64_t)p * kStampRegions + r] = st_acc[r];
  if (leader && A.tl) {
    A.tl[2 * (int64_t)p] = rt0;
    A.tl[2 * (int64_t)p + 1] = __builtin_amdgcn_s_memrealtime();
  }
  }
#endif
  if (!kSliced || !yielded) {
    if (leader) A.part_npairs[p] = np;
  }
  if constexpr (kSliced) {
    // a parked partition goes to the ring's end, unless its entry comes back abandoned: then the
    // wave keeps it (ticket -1: no claim) and takes it up from the save area like any other
    parked = yielded && !slice_publish(A, p);
    if (parked) {
      ticket = -1;
    } else {
      ticket = slice_claim(A, &p);
      parked = ticket >= A.n_part;
    }
    if (ticket < 0 && !parked) break;
  }
  } while (kSliced);
  if constexpr (kSliced) {
    // out of the queue: pack `dense` (what the one-shot launch's extra workgroups do)
    const int64_t n_grp = A.sl_dense ? (A.n_kept_sent + 63) / 64 : 0;
    while (n_grp) {
      int32_t g0 = 0;
      if (leader) g0 = (int32_t)__hip_atomic_fetch_add(&A.sl_ctl[2], (unsigned)kDenseClaim, LDDL_RLX_AGENT);
      g0 = uni(g0);
      if ((int64_t)(uint32_t)g0 >= n_grp) break;
      for (int g = 0; g < kDenseClaim && (int64_t)(uint32_t)g0 + g < n_grp; ++g)
        densify_group(((int64_t)(uint32_t)g0 + g) * 64, A.ks_start, A.ks_len, A.kscan, A.n_kept_sent,
                      A.ids, A.dense);
    }
  }
}

// the largest partition's pair count (the partition shuffle's LDS size)
__global__ void max_pairs_kernel(const int64_t* np, int64_t n, unsigned long long* out) {
  int64_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = np[i] > m ? np[i] : m;
  if (m) atomicMax(out, (unsigned long long)m);
}

struct Identity {
  const int64_t* v;
  __device__ int64_t operator()(int64_t i) const { return v[i]; }
};

// Split plan: the first kept sentence of the tail range's partitions (= the end of the head's)
// and the kept tokens before it. info[0] bounds the two ranges' dense packing, info[1] scales
// the head's counts to the suggested output capacities.
__global__ void split_info_kernel(const int64_t* kp_off, const int64_t* kd_off, const int64_t* kscan,
                                  int64_t s, int64_t* info) {
  const int64_t k = kd_off[kp_off[s]];
  info[0] = k;
  info[1] = kscan[k];
}

// part_base[s + 1 + i] = head_pairs + rel[i + 1], i in [0, n): the tail range's partitions in
// the plan's one table of first output pairs (part_base[s] = head_pairs came with the head)
__global__ void tail_part_base_kernel(const int64_t* rel, int64_t n, int64_t head_pairs,
                                      int64_t* part_base_s) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) part_base_s[1 + i] = head_pairs + rel[i + 1];
}

}  // namespace

// exclusive scan of v[0 .. n), out[n] = the total: scan_exclusive over Identity, instantiated here
// alone (the planner's pairs per partition; the native planner's pairs per unit)
hipError_t scan_i64(const int64_t* v, int64_t n, int64_t* out, int64_t* scratch, hipStream_t st) {
  return scan_exclusive(Identity{v}, n, out, scratch, st);
}

// LDDL_RNG_REPLAY planner, set-up: the slot tables, the planner's arguments (W.A) and the sizes
// of the mask pools; decides whether the launch is split into a head and a tail range.
int plan_replay_setup(lddl_pairs* P, PlanWork& W) {
  const lddl_pair_params* prm = W.prm;
  const int64_t n_part = W.n_part;
  if (prm->seq > 512) LDDL_FAIL(-1, "replay planner supports target_seq_length <= 512");
  const int64_t slots = (int64_t)prm->dup * P->n_kept_sent;
  int rc;
  if ((rc = P->mem.take(&P->desc, slots)) || (rc = P->mem.take(&P->order, slots)) ||
      (rc = W.tmp.take(&W.jseq, slots)) || (rc = W.tmp.take(&W.part_npairs, n_part + 1)))
    return rc;
  if (prm->masking && (rc = W.tmp.take(&W.spool, slots))) return rc;
  PlanArgs& A = W.A;
  fill_plan_args(A, P, W);
  A.ks_start = P->ks_start;
  A.ids = W.d_ids;
  A.n_kept_sent = dense_in_plan(W) ? P->n_kept_sent : 0;
  A.n_dense_wg = 4096;
  A.max_pred = P->max_pred;
  A.short_seq_prob = prm->short_seq_prob;
  A.seq_r64 = ((prm->seq + 63) / 64) * 64;
  A.desc = P->desc;
  A.jseq = W.jseq;
  A.spool = W.spool;
  A.part_npairs = W.part_npairs;
#ifdef LDDL_STAMPS
  if ((rc = W.tmp.take(&W.d_stamps, n_part * kStampRegions)) || (rc = W.tmp.take(&W.d_tl, n_part * 2)))
    return rc;
  LDDL_HIP(hipMemsetAsync(W.d_stamps, 0, 8 * n_part * kStampRegions, W.st));
  LDDL_HIP(hipMemsetAsync(W.d_tl, 0, 16 * n_part, W.st));
  A.stamps = W.d_stamps;
  A.tl = W.d_tl;
#endif
  // pools: decisions (int32, shuffled order) and shuffle draws (uint16), sized from the kept
  // tokens (expected use ~0.15 * 1.5 and ~1.5 times dup * tokens); a plan that outgrows them
  // reports the exact sizes and is planned again (deterministic replay)
  if ((rc = W.tmp.take(&W.pool_ctl, 4)) || (rc = P->mem.take(&P->part_base, n_part + 1))) return rc;
  PoolAttempt& L = W.pools;  // (no entries unless the plan masks)
  A.jbytes = prm->seq <= 256 ? 1 : 2;  // every draw j_i < nc <= seq - 3
  if (prm->masking && W.n_sent) {
    L.cap = (int64_t)(2.0 * prm->masked_lm_ratio * prm->dup * (double)W.n_kept_tok) +
            (int64_t)prm->dup * P->n_kept_sent / 2 + kPoolChunk * (n_part + 16);
    L.jcap = (int64_t)(1.6 * prm->dup * (double)W.n_kept_tok) + 8 * slots +
             kPoolChunk * (n_part + 16);  // + the 16-entry alignment of every pair's draws
    if (W.knobs.mask_pool >= 0) L.cap = W.knobs.mask_pool;  // tests: force a re-plan
  }
  // SlotPool keeps pool offsets as 32-bit multiples of 8 / 16 entries
  if (L.cap / 8 >= (int64_t)UINT32_MAX || L.jcap / 16 >= (int64_t)UINT32_MAX)
    LDDL_FAIL(-1, "batch too large for the mask pools (split it into smaller GPU batches)");
  A.pool_used = W.pool_ctl;
  A.overflow = reinterpret_cast<int32_t*>(W.pool_ctl + 1);
  return 0;
}

typedef void (*PlanKernel)(PlanArgs);
static PlanKernel planner_kernel(const PlanWork& W, bool sliced) {
  const bool docs_lds = W.max_docs + 1 <= (unsigned long long)kDocLds;  // document table in LDS
  if (sliced)
    return docs_lds ? (W.A.jbytes == 1 ? plan_replay_kernel<true, 1, true> : plan_replay_kernel<true, 2, true>)
                    : (W.A.jbytes == 1 ? plan_replay_kernel<false, 1, true> : plan_replay_kernel<false, 2, true>);
  return docs_lds ? (W.A.jbytes == 1 ? plan_replay_kernel<true, 1> : plan_replay_kernel<true, 2>)
                  : (W.A.jbytes == 1 ? plan_replay_kernel<false, 1> : plan_replay_kernel<false, 2>);
}

// The plan's mode (plan_replay_mode, plan_split.h: one shot, time-sliced or split at W.split.s)
// and what follows from the decision to slice: the grid, the ring and the save areas.
int choose_mode(const lddl_pairs* P, PlanWork& W) {
  // planner workgroups (one wave each) the device holds at once, of either instantiation
  auto capacity_of = [&W](bool sliced, int64_t* capacity) {
    int per_cu = 0, n_cu = 0;
    LDDL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, planner_kernel(W, sliced), 64, kPlanLds));
    LDDL_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, W.c->device));
    *capacity = (int64_t)per_cu * n_cu;
    return 0;
  };
  ReplayMode m;
  int rc = plan_replay_mode(W.n_part, W.prm->masking != 0, W.knobs.split, W.knobs.slice, capacity_of, &m);
  SlicePlan& S = W.slice;
  S.on = m.sliced;
  W.split.s = m.split;
  if (rc || !S.on) return rc;
  S.grid = std::min<int64_t>(W.n_part, W.knobs.waves > 0 ? W.knobs.waves : std::max<int64_t>(m.capacity, 1));
  const unsigned __int128 units = (unsigned __int128)(uint64_t)W.prm->dup * (uint64_t)P->n_kept_doc;
  S.ring_cap = plan_slice_ring_entries(
      W.n_part, units > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)units, W.knobs.slice);
  // tickets and dense-group claims are 32-bit counters
  if (S.ring_cap >= INT32_MAX - W.n_part || P->n_kept_sent / 64 >= INT32_MAX - (int64_t)(1 << 24))
    LDDL_FAIL(-1, "batch too large for the time-sliced plan (LDDL_PLAN_SLICE=0, or smaller GPU batches)");
  PlanArgs& A = W.A;
  if ((rc = W.tmp.take(&S.queue, 4 + ((S.ring_cap + 3) & ~(int64_t)3))) ||
      (rc = W.tmp.take(&A.sl_save, W.n_part * kSaveU64)))
    return rc;
  A.sl_ctl = S.queue;
  A.sl_ring = S.queue + 4;
  A.sl_ring_cap = (int32_t)S.ring_cap;
  A.sl_dense = W.knobs.slice_dense == 1;
  A.sl_quantum = (int32_t)std::min<int64_t>(std::max<int64_t>(W.knobs.slice, 0), INT32_MAX);
#ifdef LDDL_STAMPS
  if ((rc = W.tmp.take(&W.d_tls, 2 * (W.n_part + S.ring_cap)))) return rc;
  LDDL_HIP(hipMemsetAsync(W.d_tls, 0, 16 * (W.n_part + S.ring_cap), W.st));
  A.tls = W.d_tls;
#endif
  return 0;
}

// The pools of one planning attempt (the counters cleared on the stream first). A split plan also
// takes `mpos` here, at the pool's capacity: mpos shares the mask pool's index space, and the
// head's mask replay fills it while the tail range still allocates from the pool.
static int take_pools(lddl_pairs* P, PlanWork& W, bool split) {
  PoolAttempt& L = W.pools;
  L.mtok_try = nullptr;
  L.jpool_try = nullptr;
  int rc;
  if (W.prm->masking) {
    LDDL_HIP(hipMemsetAsync(W.pool_ctl, 0, 32, W.st));
    if ((rc = P->mem.take(&L.mtok_try, L.cap + 4)) ||
        (rc = W.tmp.take(&L.jpool_try, W.A.jbytes * (L.jcap + 16))) ||
        (split && (rc = P->mem.take(&P->mpos, L.cap + 4))))
      return rc;
  }
  W.A.mtok = L.mtok_try;
  W.A.jpool = L.jpool_try;
  W.A.pool_cap = L.cap;
  W.A.jpool_cap = L.jcap;
  return 0;
}

// The attempt stands: its blocks are the plan's. One range takes `mpos` now, at its exact size.
static int adopt_pools(lddl_pairs* P, PlanWork& W, const unsigned long long ctl[4]) {
  P->mtok = W.pools.mtok_try;
  W.jpool = W.pools.jpool_try;
  return W.split.s ? 0 : P->mem.take(&P->mpos, (int64_t)ctl[0]);
}

// The attempt is void: its blocks go back, with `mpos` and a split plan's head tables (laid out on them).
void drop_pools(lddl_pairs* P, PlanWork& W) {
  PairRange& h = P->rg[0];
  for (void* b : {(void*)W.pools.mtok_try, (void*)P->mpos, (void*)h.rec, (void*)h.tok_off, (void*)h.pos_off})
    if (b) P->mem.give(b);
  W.tmp.give(W.pools.jpool_try);
  P->mtok = nullptr;
  P->mpos = nullptr;
  W.jpool = nullptr;
  h = PairRange{};
}

void grow_pools(PlanWork& W, const unsigned long long ctl[4]) {  // exactly what this attempt needed
  W.pools.cap = (int64_t)ctl[0] + 1024;
  W.pools.jcap = (int64_t)ctl[2] + 1024;
}

// One plan_replay_kernel launch over partitions [p0, p0 + n) on `st`. with_dense: its extra
// workgroups pack the kept sentences from *dense_lo on (null: all of them).
static int launch_planner(const PlanWork& W, int64_t p0, int64_t n, hipStream_t st, bool with_dense,
                          const int64_t* dense_lo) {
  PlanArgs A = W.A;
  A.p0 = (int32_t)p0;
  A.n_part = (int32_t)n;
  A.dense_lo = dense_lo;
  if (!with_dense) A.n_kept_sent = 0;
  if (W.slice.on) {
    // The whole plan by the persistent grid. `dense` is packed by the waves that leave the queue
    // (the default), or by densify_kernel behind (LDDL_PLAN_SLICE_DENSE=0) or ahead of the
    // planner (2): the one-shot launch's tail, which hides that work, no longer exists.
    auto densify = [&]() {
      if (A.n_kept_sent) launch_densify(A.ks_start, A.ks_len, A.kscan, A.n_kept_sent, A.ids, A.dense, st);
    };
    LDDL_HIP(hipMemsetAsync(W.slice.queue, 0, 4 * (4 + ((W.slice.ring_cap + 3) & ~(int64_t)3)), st));
    if (W.knobs.slice_dense == 2) densify();
    hipLaunchKernelGGL(planner_kernel(W, true), dim3((unsigned)W.slice.grid), dim3(64), kPlanLds, st, A);
    if (W.knobs.slice_dense == 0) densify();
  } else if (const unsigned grid = (unsigned)n + (A.n_kept_sent ? (unsigned)A.n_dense_wg : 0u)) {
    hipLaunchKernelGGL(planner_kernel(W, false), dim3(grid), dim3(64), kPlanLds, st, A);
  }
  LDDL_HIP(hipGetLastError());
  return 0;
}

// The planner's one sync per range, partitions [p0, p0 + n): pairs per partition -> their first
// pairs in `table` (table[n], the range's pair count, to *n_pairs) and the largest count
// (W.max_np), read back with the pool counters (ctl) and one more copy (x_dst null: none).
static int read_back_range(PlanWork& W, int64_t p0, int64_t n, int64_t* table, int64_t* n_pairs,
                           unsigned long long ctl[4], void* x_dst = nullptr, const void* x_src = nullptr,
                           size_t x_bytes = 0) {
  hipStream_t st = W.st;
  if (!W.prm->masking) LDDL_HIP(hipMemsetAsync(W.pool_ctl, 0, 32, st));
  LDDL_HIP(scan_exclusive(Identity{W.part_npairs + p0}, n, table, W.scratch, st));
  hipLaunchKernelGGL(max_pairs_kernel, dim3(64), dim3(256), 0, st, W.part_npairs + p0, n, W.pool_ctl + 3);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipMemcpyAsync(ctl, W.pool_ctl, 32, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipMemcpyAsync(n_pairs, table + n, 8, hipMemcpyDeviceToHost, st));
  if (x_dst) LDDL_HIP(hipMemcpyAsync(x_dst, x_src, x_bytes, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  W.max_np = std::max<int64_t>(1, (int64_t)ctl[3]);
  return 0;
}

// One range: launches plan_replay_kernel (between the plan's two events) and, when a pool
// overflowed, once more with the exact sizes. attempt 1: the re-plan of a split plan.
int plan_replay_unsplit(lddl_pairs* P, PlanWork& W, int attempt) {
  int rc;
  for (; W.n_part; ++attempt) {
    if ((rc = take_pools(P, W, false))) return rc;
    LDDL_HIP(hipEventRecord(P->ev[0], W.st));
    if ((rc = launch_planner(W, 0, W.n_part, W.st, true, nullptr))) return rc;
    LDDL_HIP(hipEventRecord(P->ev[1], W.st));
    unsigned long long ctl[4];
    unsigned sl_ctl[4] = {0, 0, 0, 0};
    if ((rc = read_back_range(W, 0, W.n_part, P->part_base, &P->n_pairs, ctl, W.slice.on ? sl_ctl : nullptr,
                              W.slice.queue, 16)))
      return rc;
    P->n_slices = sl_ctl[1];
    if (!W.prm->masking) break;
    if (!ctl[1]) return adopt_pools(P, W, ctl);
    drop_pools(P, W);
    if (attempt > 0) LDDL_FAIL(-1, "mask pool overflow after resize");
    grow_pools(W, ctl);
  }
  return 0;
}

// Split plan, first half: the head range [0, s) on the caller's stream and the tail range
// [s, n_part) on the side stream, both allocating from the same pools. The tail launch keeps the
// dense-packing workgroups for its kept sentences; the head's are packed by densify_head_kernel,
// first on the caller's stream after the head planner (by then every tail workgroup that fits is
// resident). Returns after the head's sync with rg[0] = [0, s), its n_pairs, and *usable = no pool
// overflow so far: the pools then stand unless the tail overflows them (else the head's slots may
// point past the pools, nothing downstream may run on them, and the range counts no pairs).
int plan_replay_split_head(lddl_pairs* P, PlanWork& W, bool* usable) {
  SplitPlan& S = W.split;
  const int64_t n_part = W.n_part, s = S.s;
  int rc;
  // the context's side stream for the tail range: non-blocking (the caller's stream may be the
  // null stream) and of the lowest priority, so the head range's workgroups are placed first
  if (!W.c->plan_side) {
    int least = 0, greatest = 0;
    LDDL_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    LDDL_HIP(hipStreamCreateWithPriority(&W.c->plan_side, hipStreamNonBlocking, least));
  }
  hipStream_t st = W.st, side = W.c->plan_side;
  if ((rc = take_pools(P, W, true)) || (rc = W.tmp.take(&S.info, 2)) ||
      (rc = W.tmp.take(&S.tail_rel, n_part - s + 1)))
    return rc;
  LDDL_HIP(hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming));
  LDDL_HIP(hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming));
  hipLaunchKernelGGL(split_info_kernel, dim3(1), dim3(1), 0, st, P->kp_off, P->kd_off, P->kscan, s, S.info);
  LDDL_HIP(hipGetLastError());
  LDDL_HIP(hipEventRecord(P->ev[0], st));
  // the side stream starts after the compaction (and everything else queued on st so far)
  LDDL_HIP(hipEventRecord(P->ev_fork, st));
  LDDL_HIP(hipStreamWaitEvent(side, P->ev_fork, 0));
  if ((rc = launch_planner(W, 0, s, st, false, nullptr))) return rc;
  P->tail_pending = true;  // (from here every return path joins before a block goes back)
  rc = launch_planner(W, s, n_part - s, side, true, S.info);
  LDDL_HIP(hipEventRecord(P->ev_join, side));
  if (rc) return rc;
  if (P->n_kept_sent)
    launch_densify_head(P->ks_start, P->ks_len, P->kscan, P->n_kept_sent, S.info, W.d_ids, P->dense, st);
  unsigned long long ctl[4];
  if ((rc = read_back_range(W, 0, s, P->part_base, &P->rg[0].n_pairs, ctl, S.h_info, S.info, 16))) return rc;
  P->rg[0].p1 = s;
  *usable = ctl[1] == 0;
  if (!*usable) P->rg[0].n_pairs = 0;
  return *usable ? adopt_pools(P, W, ctl) : 0;
}

// Split plan, second half: joins the tail range on the planning stream and reads it back
// (rg[1].n_pairs; W.split.tail_rel: its partitions' first pairs; ctl[1] != 0: a pool overflowed).
int plan_replay_split_tail(lddl_pairs* P, PlanWork& W, unsigned long long ctl[4]) {
  P->join(W.st);
  LDDL_HIP(hipEventRecord(P->ev[1], W.st));
  return read_back_range(W, W.split.s, W.n_part - W.split.s, W.split.tail_rel, &P->rg[1].n_pairs, ctl);
}

// The tail range's partitions in the plan's table of first output pairs, behind the head's.
int tail_part_base(lddl_pairs* P, PlanWork& W) {
  const int64_t s = W.split.s, n_tail = W.n_part - s;
  if (n_tail)
    hipLaunchKernelGGL(tail_part_base_kernel, dim3((unsigned)((n_tail + 255) / 256)), dim3(256), 0,
                       W.st, W.split.tail_rel, n_tail, P->rg[0].n_pairs, P->part_base + s);
  LDDL_HIP(hipGetLastError());
  return 0;
}

#ifdef LDDL_STAMPS
// diagnostic build: region shares of plan_replay_kernel and the timeline of its partitions
int report_plan_stamps(const PlanWork& W) {
  const int64_t n_part = W.n_part;
  hipStream_t st = W.st;
  std::vector<uint64_t> h(n_part * kStampRegions);
  LDDL_HIP(hipMemcpyAsync(h.data(), W.d_stamps, 8 * h.size(), hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  double tot[kStampRegions] = {0};
  for (int64_t q = 0; q < n_part; ++q)
    for (int r = 0; r < kStampRegions; ++r) tot[r] += (double)h[q * kStampRegions + r];
  const char* names[kStampRegions] = {"plan", "cand", "shuffle_draws", "random_next", "decisions",
                                      "trunc", "final_shuffle_draws", "fy_jacobi_passes_per_window"};
  double all = 0;
  for (int r = 0; r < kStampRegions - 1; ++r) all += tot[r];
  fprintf(stderr, "[stamps] plan_replay_kernel mean cycles per partition:");
  for (int r = 0; r < kStampRegions - 1; ++r)
    fprintf(stderr, " %s=%.3g (%.1f%%)", names[r], tot[r] / n_part, 100.0 * tot[r] / (all + 1e-9));
  fprintf(stderr, " %s=%.3f\n", names[kStampRegions - 1], tot[kStampRegions - 1] / n_part / 1e6);
  // timeline (100 MHz real-time clock): partition durations and concurrency over the launch
  std::vector<uint64_t> t(2 * n_part);
  LDDL_HIP(hipMemcpyAsync(t.data(), W.d_tl, 16 * n_part, hipMemcpyDeviceToHost, st));
  LDDL_HIP(hipStreamSynchronize(st));
  uint64_t t0 = ~0ull, t1 = 0;
  std::vector<double> dur(n_part);
  for (int64_t q = 0; q < n_part; ++q) {
    t0 = std::min(t0, t[2 * q]);
    t1 = std::max(t1, t[2 * q + 1]);
    dur[q] = (t[2 * q + 1] - t[2 * q]) / 1e5;  // ms
  }
  std::vector<double> sd = dur;
  std::sort(sd.begin(), sd.end());
  const double span = (t1 - t0) / 1e5;
  fprintf(stderr, "[timeline] span %.2f ms, partition ms min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f\n",
          span, sd[0], sd[n_part / 10], sd[n_part / 2], sd[n_part * 9 / 10], sd[n_part - 1]);
  const int nb = 40;
  fprintf(stderr, "[timeline] active partitions per %.2f ms bin:", span / nb);
  for (int b = 0; b < nb; ++b) {
    const uint64_t a = t0 + (t1 - t0) * b / nb, e = t0 + (t1 - t0) * (b + 1) / nb;
    double act = 0;  // partition-time inside the bin / bin length
    for (int64_t q = 0; q < n_part; ++q) {
      const uint64_t s0 = std::max(a, t[2 * q]), s1 = std::min(e, t[2 * q + 1]);
      if (s1 > s0) act += (double)(s1 - s0);
    }
    fprintf(stderr, " %.0f", act / (double)(e - a));
  }
  fprintf(stderr, "\n[timeline] start ms of partitions by index decile:");
  for (int k = 0; k <= 10; ++k) {
    const int64_t q = std::min<int64_t>(n_part - 1, n_part * k / 10);
    fprintf(stderr, " %.1f", (t[2 * q] - t0) / 1e5);
  }
  fprintf(stderr, "\n");
  if (W.slice.on) {  // the slices (one per ticket): how many waves were planning in every bin
    const int64_t n_tk = n_part + W.slice.ring_cap;
    std::vector<uint64_t> ts(2 * n_tk);
    LDDL_HIP(hipMemcpyAsync(ts.data(), W.d_tls, 16 * n_tk, hipMemcpyDeviceToHost, st));
    LDDL_HIP(hipStreamSynchronize(st));
    std::vector<double> sl;
    for (int64_t q = 0; q < n_tk; ++q)
      if (ts[2 * q + 1]) sl.push_back((ts[2 * q + 1] - ts[2 * q]) / 1e5);
    std::sort(sl.begin(), sl.end());
    if (!sl.empty())
      fprintf(stderr, "[timeline] %zu slices on %lld waves, slice ms min %.2f p50 %.2f p90 %.2f max %.2f\n",
              sl.size(), (long long)W.slice.grid, sl[0], sl[sl.size() / 2], sl[sl.size() * 9 / 10], sl.back());
    fprintf(stderr, "[timeline] active waves (slices) per %.2f ms bin:", span / nb);
    for (int b = 0; b < nb; ++b) {
      const uint64_t a = t0 + (t1 - t0) * b / nb, e = t0 + (t1 - t0) * (b + 1) / nb;
      double act = 0;
      for (int64_t q = 0; q < n_tk; ++q) {
        if (!ts[2 * q + 1]) continue;
        const uint64_t s0 = std::max(a, ts[2 * q]), s1 = std::min(e, ts[2 * q + 1]);
        if (s1 > s0) act += (double)(s1 - s0);
      }
      fprintf(stderr, " %.0f", act / (double)(e - a));
    }
    fprintf(stderr, "\n");
  }
  return 0;
}
#endif

}  // namespace lddl
