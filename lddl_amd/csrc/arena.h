// The device-memory arena for the library's per-call temporaries, and the owners of its blocks.
// Ownership rule: a C-ABI function never holds a bare DevArena::Block. One temporary is an
// ArenaTmp, several (or a plan's) are an ArenaScope, so every return path gives the blocks back.
// (Host-only: the HIP runtime API and the standard library, so a CPU program can test it.)
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "common.h"

namespace lddl {
// Device memory cache for the library's per-call temporaries (pair plans). Blocks are plain
// hipMalloc allocations that are never returned while the context lives: a released block goes
// to the free list with an event recorded on the releasing stream, and a later request takes the
// smallest free block that fits (up to 1.5x the request; a stream other than the releasing one
// waits on the event first). A batch-per-step workload therefore allocates only in its first
// step. (The stream-ordered HIP pool that this replaces showed 0.4-2 s hipMallocAsync calls
// once torch's caching allocator held a large share of HBM.)
//
// With an external allocator set (lddl_ctx_set_allocator: the host hands in its own device
// allocator, e.g. PyTorch's caching allocator), blocks come from and go straight back to it and
// nothing is cached here, so one pool owns HBM.
class DevArena {
 public:
  typedef void* (*AllocFn)(size_t bytes, void* stream, void* user);
  typedef void (*FreeFn)(void* p, void* stream, void* user);
  struct Block {
    void* p = nullptr;
    size_t size = 0;
    hipEvent_t ev = nullptr;
    hipStream_t st = nullptr;
    bool ext = false;  // from the external allocator
  };
  void set_external(AllocFn a, FreeFn f, void* user) {
    trim();
    std::lock_guard<std::mutex> g(mu_);
    alloc_ = a;
    free_fn_ = f;
    user_ = user;
  }
  hipError_t take(size_t bytes, hipStream_t st, Block& out) {
    if (alloc_) {
      out = Block{};
      out.size = bytes ? bytes : 16;
      out.p = alloc_(out.size, (void*)st, user_);
      out.ext = true;
      out.st = st;
      return out.p ? hipSuccess : hipErrorOutOfMemory;
    }
    const size_t want = round_up(bytes);
    {
      std::lock_guard<std::mutex> g(mu_);
      size_t best = free_.size();
      for (size_t i = 0; i < free_.size(); ++i)
        if (free_[i].size >= want && free_[i].size <= want + want / 2 &&
            (best == free_.size() || free_[i].size < free_[best].size))
          best = i;
      if (best < free_.size()) {
        out = free_[best];
        free_.erase(free_.begin() + (ptrdiff_t)best);
        if (out.st != st && out.ev) (void)hipStreamWaitEvent(st, out.ev, 0);
        return hipSuccess;
      }
    }
    out = Block{};
    out.size = want;
    hipError_t e = hipMalloc(&out.p, want);
    if (e != hipSuccess) {  // release the cached blocks and retry once
      (void)hipGetLastError();
      trim();
      e = hipMalloc(&out.p, want);
    }
    return e;
  }
  void give(Block b, hipStream_t st) {
    if (!b.p) return;
    if (b.ext) {
      // a stream-ordered external pool (torch's caching allocator) reuses the block on the stream
      // it was allocated on: when the last use was on another stream, that stream is ordered
      // after it first, so no later allocation there can overwrite the block while it is in use
      if (st != b.st) {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
          (void)hipEventRecord(ev, st);
          (void)hipStreamWaitEvent(b.st, ev, 0);
          (void)hipEventDestroy(ev);
        }
      }
      if (free_fn_) free_fn_(b.p, (void*)b.st, user_);
      return;
    }
    if (!b.ev) (void)hipEventCreateWithFlags(&b.ev, hipEventDisableTiming);
    if (b.ev) (void)hipEventRecord(b.ev, st);
    b.st = st;
    std::lock_guard<std::mutex> g(mu_);
    free_.push_back(b);
  }
  void trim() {  // free every cached block (after the work that used them)
    std::lock_guard<std::mutex> g(mu_);
    for (Block& b : free_) {
      if (b.ev) {
        (void)hipEventSynchronize(b.ev);
        (void)hipEventDestroy(b.ev);
      }
      (void)hipFree(b.p);
    }
    free_.clear();
  }
  ~DevArena() { trim(); }

 private:
  static size_t round_up(size_t b) {  // 2 MiB granules, 1/16 of the size above 32 MiB
    size_t g = (size_t)2 << 20;
    if (b > ((size_t)32 << 20)) g = std::max(g, b / 16);
    return (b + g - 1) / g * g;
  }
  std::mutex mu_;
  std::vector<Block> free_;
  AllocFn alloc_ = nullptr;
  FreeFn free_fn_ = nullptr;
  void* user_ = nullptr;
};

// A temporary from the arena for the duration of one C-ABI call (returned on `st`).
struct ArenaTmp {
  DevArena* a;
  hipStream_t st;
  DevArena::Block b{};
  ArenaTmp(DevArena* arena, hipStream_t stream) : a(arena), st(stream) {}
  hipError_t take(size_t bytes) { return a->take(bytes, st, b); }
  template <typename T>
  T* as() const { return static_cast<T*>(b.p); }
  ~ArenaTmp() { a->give(b, st); }
};

// Owner of any number of blocks from one arena, taken on one stream: a plan's tables, or the
// temporaries of a call that needs several. What is still held when the scope dies goes back on
// that stream; release(st) gives everything back on another (the stream of the last use).
class ArenaScope {
 public:
  ArenaScope(DevArena* arena, hipStream_t stream) : a_(arena), st_(stream) {}
  ArenaScope(const ArenaScope&) = delete;
  ArenaScope& operator=(const ArenaScope&) = delete;
  ~ArenaScope() { release(st_); }
  // n elements of T (one when n <= 0); on failure sets the error and returns its code
  template <typename T>
  int take(T** p, int64_t n) {
    DevArena::Block b;
    LDDL_HIP(a_->take(sizeof(T) * (size_t)(n > 0 ? n : 1), st_, b));
    *p = static_cast<T*>(b.p);
    blocks_.push_back(b);
    return 0;
  }
  void give(void* p) {  // return one block early
    for (size_t i = 0; i < blocks_.size(); ++i)
      if (blocks_[i].p == p) {
        a_->give(blocks_[i], st_);
        blocks_.erase(blocks_.begin() + (ptrdiff_t)i);
        return;
      }
  }
  void release(hipStream_t st) {
    for (DevArena::Block& b : blocks_) a_->give(b, st);
    blocks_.clear();
  }

 private:
  DevArena* a_;
  hipStream_t st_;
  std::vector<DevArena::Block> blocks_;
};
}  // namespace lddl
