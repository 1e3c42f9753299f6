// What the units of the pair stage share (pairs.hip, pairs_*.hip): the records the stages hand
// to each other, the plan's state (PlanWork, with a struct of its own for a replay plan's pools,
// slice, split and range temporaries), and the host functions of each stage. Kernels and their
// device helpers are private to their unit (an anonymous namespace there, as in collate_dev.h);
// the types here appear in the stage functions' signatures, so they live in namespace lddl proper.
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>

#include "common.h"
#include "ctx.h"
#include "device.h"
#include "lddl_amd.h"
#include "pair_knobs.h"
#include "plan_split.h"
#include "scan.h"

namespace lddl {

struct alignas(16) PairDesc {
  int64_t a_ks;     // kept-sentence index where A's chunk starts
  int64_t b_ks;     // kept-sentence index where B's span starts
  int32_t a_front;  // tokens truncated from the front of A's concatenated sentences
  int32_t na;       // tokens kept in A
  int32_t b_front;
  int32_t nb_rn;    // tokens kept in B | is_random_next << 31
};

// Replay masking, per planner slot: where the pair's decisions (mask pool, entries moff8 * 8 ..)
// and shuffle draws (draw pool, joff16 * 16 ..) are, and how many. One 16-byte record, one store.
struct alignas(16) SlotPool {
  uint32_t moff8;   // mask-pool offset / 8 (regions are 8-entry aligned)
  uint32_t joff16;  // draw-pool offset / 16 (regions are 16-entry aligned)
  int32_t nmask;    // num_to_predict
  int32_t ncand;    // candidates (len(A) + len(B) minus literal [CLS]/[SEP])
};

constexpr int32_t kKeep = -1;  // mask decision "keep the original token" (pretrain.py:215-216)

// Diagnostic build only (-DLDDL_STAMPS): per-region s_memtime sums of the planner.
#ifdef LDDL_STAMPS
constexpr int kStampRegions = 8;
#define STAMP_T() __builtin_amdgcn_s_memtime()
#define STAMP_ADD(r, t0)                   \
  do {                                     \
    const uint64_t t1_ = STAMP_T();        \
    st_acc[r] += t1_ - (t0);               \
    t0 = t1_;                              \
  } while (0)
#else
#define STAMP_T() 0ull
#define STAMP_ADD(r, t0) ((void)0)
#endif

// Token ids of the pair tables (the dense kept tokens, the sample tokens and labels): 2 bytes each
// when the vocab fits uint16 (lddl_ctx::id_bytes), else 4. The hot reader (gather_kernel) is
// templated on the type; the rare paths read through this runtime-width view.
struct IdPtr {
  void* p;
  int32_t ib;
  __device__ int32_t ld(int64_t i) const {
    return ib == 2 ? (int32_t)static_cast<const uint16_t*>(p)[i] : static_cast<const int32_t*>(p)[i];
  }
  __device__ void st(int64_t i, int32_t v) const {
    if (ib == 2) static_cast<uint16_t*>(p)[i] = (uint16_t)v;
    else static_cast<int32_t*>(p)[i] = v;
  }
};

struct PlanArgs {
  // kept corpus
  const int64_t* kscan;  // dense token offset of each kept sentence
  const int32_t* ks_len;
  const int64_t* kd_off;
  const int64_t* kp_off;
  const int64_t* ks_start;  // kept sentence k's pieces at ids[ks_start[k] ...]: the tokenizer's
  const int32_t* ids;       // layout (`dense` is filled by this launch's tail workgroups)
  IdPtr dense;              // out: kept tokens, packed (densify_group)
  int64_t n_kept_sent;
  int32_t n_part, n_dense_wg;  // workgroups >= n_part fill `dense`
  // one launch plans partitions [p0, p0 + n_part) (a split plan: a head and a tail launch); its
  // dense workgroups pack kept sentences [*dense_lo, n_kept_sent) (null: from 0)
  int32_t p0;
  const int64_t* dense_lo;
  const int64_t* part_seed;
  // params
  int32_t seq, dup, masking, vocab_size, cls_id, sep_id, mask_id, max_pred;
  double short_seq_prob, ratio;
  uint64_t k_short;  // random() < short_seq_prob  <=>  N < k_short = ceil(short_seq_prob * 2^53)
  int32_t seq_r64;   // seq rounded up to a multiple of 64
  // outputs, slot base of partition p = dup * kd_off[kp_off[p]]
  PairDesc* desc;
  int32_t* jseq;       // per slot: j_i draws of the final partition shuffle
  SlotPool* spool;     // per slot (masking)
  int32_t* mtok;       // mask pool: slot s's decisions at 8 * moff8 .. + nmask (shuffled order)
  void* jpool;         // draw pool: j_i of random.shuffle(cand_indexes) at 16 * joff16 + i
  int32_t jbytes;      // 1 (target_seq_length <= 256: every j_i < 256) or 2 bytes per draw
  unsigned long long* pool_used;  // [0] masks, [1] overflow flag, [2] draws
  int64_t pool_cap, jpool_cap;
  int32_t* overflow;   // set when the pool is too small (the host re-plans with a larger one)
  int64_t* part_npairs;
  uint64_t* stamps;  // diagnostic build: [n_part][8]
  uint64_t* tl;      // diagnostic build: [n_part][2] s_memrealtime at start / end (100 MHz)
  // time-sliced mode (plan_replay_kernel<.., true>; see "The time-sliced mode", replay_slice.h)
  unsigned* sl_ctl;   // [0] tickets claimed, [1] ring entries reserved (= hand-offs),
                      // [2] dense groups claimed, [3] unused; zeroed with the ring on every launch
  unsigned* sl_ring;  // [sl_ring_cap] 0 = not published, partition + 1, or kRingAbandoned
  uint64_t* sl_save;  // [n_part][kSaveU64] a parked partition's state
  int32_t sl_ring_cap;
  int32_t sl_dense;    // 1: the waves that leave the queue pack `dense`
  int32_t sl_quantum;  // documents per slice; 0: 1/kPlanSliceK of the partition's dup * documents
  uint64_t* tls;       // diagnostic build: [n_part + sl_ring_cap][2] slice start / end by ticket
};

// The pair maps of map_pairs_kernel, written by the partition shuffle's last pass (any may be
// null): src[q] the slot of output pair q, slots[i] the i-th slot in planner order, dstq[i] the
// output position of the i-th pair in planner order; part_base[p] = the partition's first pair.
struct PairMaps {
  const int64_t* part_base;
  int64_t *src, *slots, *dstq;
};

// Per output pair, everything the gather needs, in output order: the A and B windows in the dense
// token array, the lengths and is_random_next, and the masks' place in the mask pool. Built one
// lane per pair (src -> descriptor -> sentence offsets: every load of a wave in flight at once),
// so the scans and the gather read it front to back instead of chasing src[q] themselves.
struct alignas(16) GatherRec {
  int64_t aoff, boff, moff;
  int32_t na, nb_rn, nm, pad;
};

// The mask pools of one planning attempt; take_, adopt_, drop_ and grow_pools (pairs.hip) are its
// four ends. An attempt that overflows a pool reports the exact sizes for the next one.
struct PoolAttempt {
  int64_t cap = 0, jcap = 0;    // entries: decisions, shuffle draws
  int32_t* mtok_try = nullptr;  // this attempt's blocks
  uint8_t* jpool_try = nullptr;
};
struct SlicePlan {  // the time-sliced plan (one range)
  bool on = false;
  unsigned* queue = nullptr;       // 4 control words + the ring, zeroed before every launch
  int64_t ring_cap = 0, grid = 0;  // the ring's entries; the persistent grid
};
struct SplitPlan {          // (means something only while s != 0)
  int64_t s = 0;            // partitions of the head range (0: one range)
  int64_t* info = nullptr;  // split_info_kernel's two values, and their host copies
  int64_t h_info[2] = {0, 0};
  int64_t* tail_rel = nullptr;  // the tail partitions' first pairs, relative to the range
};
struct RangeTmp {  // a range's temporaries: shuffle_partitions (M), layout_* (pcnt, scr2)
  PairMaps M{nullptr, nullptr, nullptr, nullptr};
  int2* pcnt = nullptr;
  int64_t* scr2 = nullptr;
};

// What one planning stage hands to the next: the inputs of the call, host values read back, and
// device temporaries that no later call on the plan reads. The temporaries come from `tmp`,
// today the plan's own scope (they live until lddl_pairs_destroy); a scope local to
// lddl_pairs_plan would return them when planning ends.
// (A split plan keeps it between its head and tail calls, lddl_pairs::work.)
struct PlanWork {
  lddl_ctx* c;
  const lddl_pair_params* prm;  // the plan's own copy (lddl_pairs::prm)
  const int32_t* d_ids;
  const int64_t* d_part_seed;
  int64_t n_sent, n_part;
  hipStream_t st;
  ArenaScope& tmp;
  PlanKnobs knobs;
  PlanWork(lddl_ctx* c, const lddl_pair_params* prm, const int32_t* d_ids, const int64_t* d_part_seed,
           int64_t n_sent, int64_t n_part, hipStream_t st, ArenaScope& tmp, const PlanKnobs& knobs)
      : c(c), prm(prm), d_ids(d_ids), d_part_seed(d_part_seed), n_sent(n_sent), n_part(n_part), st(st),
        tmp(tmp), knobs(knobs) {}
  // compact_inputs
  int64_t* scratch = nullptr;  // scan scratch of the compaction and of the re-plan loop
  int64_t n_kept_tok = 0;
  unsigned long long max_docs = 0;  // kept documents of the largest partition
  // plan_replay
  int32_t* jseq = nullptr;
  int64_t* part_npairs = nullptr;
  SlotPool* spool = nullptr;
  void* jpool = nullptr;
  int64_t max_np = 1;  // pairs of the largest partition
  // the planner launch, kept for the tail call and the re-plan
  PlanArgs A{};
  unsigned long long* pool_ctl = nullptr;  // [0] masks used, [1] overflow flag, [2] draws used, [3] max pairs
  PoolAttempt pools;
  SlicePlan slice;
  SplitPlan split;
  RangeTmp rt;
#ifdef LDDL_STAMPS
  uint64_t *d_stamps = nullptr, *d_tl = nullptr, *d_tls = nullptr;
#endif
};

// Output pairs of partitions [p0, p1) of a plan: pair q of the range is output pair pair0 + q,
// its tokens start at tok0 + tok_off[q] and its masks at pos0 + pos_off[q].
struct PairRange {
  int64_t p0 = 0, p1 = 0;
  int64_t n_pairs = 0, n_tokens = 0, n_masked = 0;
  int64_t pair0 = 0, tok0 = 0, pos0 = 0;
  GatherRec* rec = nullptr;  // per output pair (pair_prep_kernel / fy_resolve_kernel)
  int64_t *tok_off = nullptr, *pos_off = nullptr;  // [n_pairs + 1]
};

}  // namespace lddl

// Device-resident plan of one batch of partitions (library-owned temporaries).
struct lddl_pairs {
  int32_t masking = 0, max_pred = 0, seq = 0, cls_id = -1, sep_id = -1;
  int64_t n_part = 0, n_pairs = 0, n_tokens = 0, n_masked = 0, n_kept_sent = 0, n_kept_doc = 0;
  int64_t n_slices = 0;  // hand-offs of a time-sliced plan (0: not sliced, or no partition parked)
  // every device block of the plan, from the context's arena (the context outlives its plans);
  // lddl_pairs_destroy gives them back on its stream, a plan dropped while planning on the
  // planning stream
  lddl::ArenaScope mem;
  // views
  int64_t *ks_start = nullptr, *kd_off = nullptr, *kp_off = nullptr, *kscan = nullptr;
  int32_t* ks_len = nullptr;
  lddl::IdPtr dense{nullptr, 4};  // kept tokens, packed in kept-sentence order (id_bytes each)
  lddl::PairDesc* desc = nullptr;
  int32_t *order = nullptr, *nmask = nullptr, *mtok = nullptr;
  uint16_t* mpos = nullptr;
  int64_t* moff = nullptr;
  int64_t* src = nullptr;
  // The output pairs' tables. One range covers the plan; a split replay plan has two, the head
  // and the tail partitions' pairs, each with blocks sized by its own pair count.
  lddl::PairRange rg[2];
  int n_rg = 1;
  int64_t* part_base = nullptr;  // [n_part + 1] first output pair of each partition
  // first planner launch .. last planner range complete (on the planning stream, after the join)
  hipEvent_t ev[2] = {nullptr, nullptr};
  // split plan: the tail launch runs on the context's side stream between ev_fork (recorded on
  // the planning stream) and ev_join; until the planning stream has waited for ev_join
  // (tail_pending) no block of the plan may go back
  hipStream_t st;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool tail_pending = false;
  bool head_valid = false;  // the head range's tables (and what was gathered from them) stand
  lddl_pair_params prm{};
  std::unique_ptr<lddl::PlanWork> work;  // between the head and the tail call

  lddl_pairs(lddl::DevArena* arena, hipStream_t stream) : mem(arena, stream), st(stream) {}
  // order `on` after the tail launch (before the plan's blocks go back on it)
  void join(hipStream_t on) {
    if (tail_pending) (void)hipStreamWaitEvent(on, ev_join, 0);
    tail_pending = false;
  }
  ~lddl_pairs() {
    join(st);  // (then `mem` gives the blocks back on st)
    for (hipEvent_t e : {ev[0], ev[1], ev_fork, ev_join})
      if (e) (void)hipEventDestroy(e);
  }
};

namespace lddl {

// replay mode: the planner launch's tail workgroups pack `dense` (plan_replay_kernel)
inline bool dense_in_plan(const PlanWork& W) { return W.prm->rng == LDDL_RNG_REPLAY && W.n_part > 0; }

// ceil(p * 2^53): random() < p  <=>  N < this (N = 53-bit integer behind random())
inline uint64_t short_threshold(double p) {
  if (!(p > 0)) return 0;
  if (p >= 1) return 1ull << 53;
  return (uint64_t)ceil(ldexp(p, 53));
}

// the kept corpus and the call's parameters, as both planners' kernels take them
template <typename Args>
inline void fill_plan_args(Args& A, const lddl_pairs* P, const PlanWork& W) {
  A.kscan = P->kscan;
  A.ks_len = P->ks_len;
  A.kd_off = P->kd_off;
  A.kp_off = P->kp_off;
  A.dense = P->dense;
  A.part_seed = W.d_part_seed;
  A.n_part = (decltype(A.n_part))W.n_part;
  A.seq = W.prm->seq;
  A.dup = W.prm->dup;
  A.masking = W.prm->masking;
  A.vocab_size = W.c->vocab_size;
  A.cls_id = P->cls_id;
  A.sep_id = P->sep_id;
  A.mask_id = W.c->tab.special_id[kMask];
  A.ratio = W.prm->masked_lm_ratio;
  A.k_short = short_threshold(W.prm->short_seq_prob);
}

// ---- the stages: each function is defined in the unit of the kernels it launches ----
// pairs_compact.hip
int compact_inputs(lddl_pairs* P, PlanWork& W, const int64_t* d_sent_off, const int32_t* d_sent_len,
                   const int64_t* d_doc_sent_off, int64_t n_doc, const int64_t* d_part_doc_off);
// pairs_native.hip
int plan_native(lddl_pairs* P, PlanWork& W);
// pairs.hip (the replay planner)
int plan_replay_setup(lddl_pairs* P, PlanWork& W);
int choose_mode(const lddl_pairs* P, PlanWork& W);
void drop_pools(lddl_pairs* P, PlanWork& W);
void grow_pools(PlanWork& W, const unsigned long long ctl[4]);
int plan_replay_unsplit(lddl_pairs* P, PlanWork& W, int attempt);
int plan_replay_split_head(lddl_pairs* P, PlanWork& W, bool* usable);
int plan_replay_split_tail(lddl_pairs* P, PlanWork& W, unsigned long long ctl[4]);
int tail_part_base(lddl_pairs* P, PlanWork& W);
#ifdef LDDL_STAMPS
int report_plan_stamps(const PlanWork& W);
#endif
// the scan over Identity (pairs.hip) has a caller in another unit; it has its one instantiation
// and its one launcher there (no kernel symbol is shared between code objects)
hipError_t scan_i64(const int64_t* v, int64_t n, int64_t* out, int64_t* scratch, hipStream_t st);
// pairs_densify.hip: the dense packing where no planner launch does it
void launch_densify(const int64_t* ks_start, const int32_t* ks_len, const int64_t* kscan, int64_t n,
                    const int32_t* ids, IdPtr dense, hipStream_t st);
void launch_densify_head(const int64_t* ks_start, const int32_t* ks_len, const int64_t* kscan, int64_t n,
                         const int64_t* n_ptr, const int32_t* ids, IdPtr dense, hipStream_t st);
// pairs_shuffle.hip
int shuffle_partitions(lddl_pairs* P, PlanWork& W, const PairRange& r, const int64_t* rel_base);
// pairs_layout.hip
int layout_pairs(lddl_pairs* P, PlanWork& W);
int layout_replay(lddl_pairs* P, PlanWork& W, PairRange& r);
// pairs_gather.hip
int emit_ranges(lddl_pairs* P, int r0, int r1, void* stream, void* d_tokens, int64_t* d_tok_off,
                int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab, int64_t* d_pos_off);

}  // namespace lddl
