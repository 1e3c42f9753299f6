// The replay planner's time-sliced queue (pairs.hip, plan_replay_kernel<.., true>): its protocol,
// the layout of a parked partition's save area with the names of its header words, the two queue
// operations (slice_claim, slice_publish) and the planner's LDS size, which is made of the same
// constants. Device code of one unit (anonymous namespace); the host side of a sliced plan
// (choose_mode, pairs.hip) sizes the save areas and the launch from the constants here.
#pragma once
#include "replay_rng.h"  // kN, kLook, uni

namespace lddl {
namespace {

constexpr int kDocLds = 512;  // partitions with <= this many documents cache offsets in LDS

// The time-sliced mode (kSliced; a one-range plan of more partitions than the device holds
// waves). The grid is persistent one-wave workgroups, as many as the device holds. A wave plans
// a partition for a quantum of documents, parks it at the document boundary and takes the next
// item of a global FIFO, so every partition gets slice k before any gets slice k + 1 and all
// the chains end together, with every wave slot busy until then.
//   Tickets, all claimed by a returning add on sl_ctl[0], the first one when the wave starts: a
//   workgroup owns no work by its index, so one that becomes resident late (measured with the
//   first tickets bound to the workgroup index: 1,024 of 7,168 started when the others left and
//   planned their partitions alone, 152 ms) finds the queue as it then is. Ticket t < n_part is
//   the fresh partition t (seeded as in the one-shot mode), ticket n_part + r is entry r of a
//   ring that never wraps (the host sizes it from the quantum: plan_slice_ring_entries).
//   Parking. The wave writes the partition's state (the MT block with its look-ahead, mti, the
//   loop position, np and the partition's pool chunks: kSaveU64 granules) to the partition's save
//   area with write-through agent-scope stores, drains them (s_waitcnt vmcnt(0)), reserves a ring
//   index with one returning add on sl_ctl[1] and publishes partition + 1 there by an atomic
//   exchange. Then it claims its next ticket.
//   Claiming. The claimant of ring entry r exchanges kRingAbandoned into it. A partition id
//   coming back is its work item: one agent-scope acquire, then the state is read by vector loads
//   (lane-indexed addresses, through LDS; the uniform words become scalars by readfirstlane). Zero
//   coming back (after kPopTries looks: the entry is reserved but not yet written, or the ring is
//   empty) means the wave leaves the queue for good.
//   No wave waits for another, and nothing is lost: the exchanges on one ring word are totally
//   ordered, so either the claimant sees the partition id and owns the partition, or the
//   publisher sees kRingAbandoned and keeps its partition for another slice (it alone ever held
//   it). Every ticket below the final sl_ctl[0] has exactly one claimant, and the final count
//   covers every published entry: each slice end (a parking that was not handed back, or a
//   finished partition) is followed by one claim, which makes n_part + published - abandoned
//   claims on top of the waves' first ones, and no more entries are ever abandoned than there are
//   waves (a wave abandons one entry, then leaves). So no workgroup's progress depends on another
//   being resident, and the launch ends whatever the dispatch order.
//   The pool chunks belong to the partition here (parked with it), not to the wave: the pools'
//   total use is then the same whichever wave plans which slice, which the exact-size re-plan
//   after a pool overflow relies on.
//   A wave that leaves the queue packs `dense`: groups of kept sentences claimed from sl_ctl[2].
constexpr int kSaveHdr = 16;                            // header words behind the MT block
constexpr int kSaveU64 = (kN + kLook + kSaveHdr) / 2;   // 8-byte granules per parked partition
constexpr int kPopTries = 4;                            // looks at a ring entry that reads zero
constexpr unsigned kRingAbandoned = 0xFFFFFFFFu;
constexpr int kDenseClaim = 4;                          // 64-sentence groups per claim
static_assert((kN + kLook + kSaveHdr) % 2 == 0 && kSaveHdr <= kDocLds, "save area layout");

// The header words of a parked partition, by name: the parking step writes them and the take-up
// reads them (both in plan_replay_kernel). 64-bit values lie as two words (Lo, Hi).
enum ParkWord : int {
  kParkMti,        // WaveRng::mti
  kParkDp,         // the loop position: duplicate pass,
  kParkDi,         // document
  kParkNpLo,       // np, the pairs planned so far (its high word: kParkNpHi)
  kParkPoolLo,     // the mask pool chunk: next entry
  kParkPoolHi,
  kParkPoolLeft,   // entries left
  kParkJpoolLo,    // the shuffle-draw pool chunk: next entry
  kParkJpoolHi,
  kParkJpoolLeft,  // entries left
  kParkFits,       // bit 0: the mask pool chunk lies inside the pool, bit 1: the draw pool chunk
  kParkNpHi,
  kParkWords       // the words in use
};
static_assert(kParkWords <= kSaveHdr, "parked header");

// ~4.8 KB of LDS per planner workgroup (the MT block with its look-ahead, the document table or
// a parked header in its place): 7 waves/SIMD fit
constexpr size_t kPlanLds = 4 * (kN + kLook) + 4 * (kDocLds + 4) + 16;

#define LDDL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// Claims the wave's next ticket (uniform): -1 = leave the queue, else the ticket, with *part the
// partition to plan (fresh when ticket < n_part, else parked).
__device__ inline int32_t slice_claim(const PlanArgs& A, int32_t* part) {
  int32_t t_out = -1, p_out = 0;
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(&A.sl_ctl[0], 1u, LDDL_RLX_AGENT);
    if (t < (unsigned)A.n_part) {
      t_out = (int32_t)t;
      p_out = (int32_t)t;
    } else if (t - (unsigned)A.n_part < (unsigned)A.sl_ring_cap) {
      unsigned* e = A.sl_ring + (t - (unsigned)A.n_part);
      for (int tries = 1; tries < kPopTries; ++tries) {  // (bounded: then the exchange decides)
        if (__hip_atomic_load(e, LDDL_RLX_AGENT) != 0) break;
        __builtin_amdgcn_s_sleep(4);
      }
      const unsigned v = __hip_atomic_exchange(e, kRingAbandoned, LDDL_RLX_AGENT);
      if (v != 0 && v != kRingAbandoned) {
        t_out = (int32_t)t;
        p_out = (int32_t)(v - 1);
      }
    }
  }
  *part = uni(p_out);
  return uni(t_out);
}

// Publishes the parked partition p (its state is stored and drained). true: handed on; false: the
// entry had been abandoned (or the ring is full), the wave keeps the partition.
__device__ inline bool slice_publish(const PlanArgs& A, int32_t p) {
  int32_t on = 0;
  if (threadIdx.x == 0) {
    const unsigned r = __hip_atomic_fetch_add(&A.sl_ctl[1], 1u, LDDL_RLX_AGENT);
    if (r < (unsigned)A.sl_ring_cap)
      on = __hip_atomic_exchange(A.sl_ring + r, (unsigned)p + 1u, LDDL_RLX_AGENT) == 0;
  }
  // the publish is complete before the wave's own claim reads the queue
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return uni(on) != 0;
}

}  // namespace
}  // namespace lddl
