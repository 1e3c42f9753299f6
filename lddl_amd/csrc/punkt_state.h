// The Punkt state of a context: the device tables lddl_punkt_set_params uploaded (punkt.hip owns
// them) and the segmentation pending between lddl_segment_count and lddl_segment_fill
// (segment.hip).
#pragma once
#include <memory>

#include "arena.h"
#include "punkt_classes.h"

// What lddl_segment_count leaves for lddl_segment_fill. The scope owns every block: dropping the
// object gives them back to the arena (on the counting stream unless released on another).
struct PendingSeg {
  lddl::ArenaScope mem;
  int32_t *cand = nullptr, *ccnt = nullptr, *rs_rel = nullptr, *cnt = nullptr, *fdoc = nullptr;
  int64_t *coff = nullptr, *dso = nullptr, *scratch = nullptr, *fq = nullptr, *fbound = nullptr;
  const int64_t* doc_off = nullptr;
  int64_t n_doc = 0;
  PendingSeg(lddl::DevArena* arena, hipStream_t st) : mem(arena, st) {}
};

struct lddl_punkt_state {
  lddl::PunktTab tab{};  // all null until the first lddl_punkt_set_params
  // the segmentation between lddl_segment_count and lddl_segment_fill (null: none pending)
  std::unique_ptr<PendingSeg> pending;
};
