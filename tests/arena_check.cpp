// CPU check of the arena's block owners (csrc/arena.h): ArenaScope and ArenaTmp over a counting
// external allocator backed by malloc / free. Exits non-zero unless every block was freed
// exactly once and none is live at the end. Built with -fsanitize=address,undefined by
// tests/test_arena.py; needs no GPU (with an external allocator and one stream the arena makes
// no HIP call).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "arena.h"

namespace lddl {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace lddl

using namespace lddl;

static std::map<void*, size_t> g_live;  // block -> bytes
static int g_allocs = 0, g_frees = 0, g_bad = 0;
static size_t g_fail_above = ~(size_t)0;  // requests larger than this fail (out of memory)

static void* count_alloc(size_t bytes, void*, void*) {
  if (bytes > g_fail_above) return nullptr;
  void* p = malloc(bytes);
  g_live[p] = bytes;
  ++g_allocs;
  return p;
}

static void count_free(void* p, void*, void*) {
  if (!g_live.erase(p)) {
    fprintf(stderr, "block %p freed twice or never allocated\n", p);
    ++g_bad;
    return;
  }
  ++g_frees;
  free(p);
}

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      ++g_bad;                                                      \
    }                                                               \
  } while (0)

// takes three blocks, then fails the fourth: the early return leaves them to the scope
static int early_return(DevArena* a) {
  ArenaScope s(a, nullptr);
  int32_t* x;
  int64_t *y, *z, *big;
  int rc;
  if ((rc = s.take(&x, 10)) || (rc = s.take(&y, 3)) || (rc = s.take(&z, 0))) return rc;
  CHECK(g_live.size() == 3);
  g_fail_above = 1 << 20;
  if ((rc = s.take(&big, 1 << 20))) return rc;
  CHECK(!"the oversized take must fail");
  return 0;
}

int main() {
  DevArena arena;
  arena.set_external(count_alloc, count_free, nullptr);
  {  // sizes, n = 0, writes across each block (the sanitizer checks the bounds)
    ArenaScope s(&arena, nullptr);
    uint8_t* a;
    int32_t* b;
    int64_t *c, *d;
    CHECK(s.take(&a, 7) == 0 && s.take(&b, 100) == 0 && s.take(&c, 0) == 0 && s.take(&d, -5) == 0);
    CHECK(g_live.size() == 4);
    CHECK(g_live[a] == 7 && g_live[b] == 400 && g_live[c] == 8 && g_live[d] == 8);
    for (int i = 0; i < 7; ++i) a[i] = 1;
    for (int i = 0; i < 100; ++i) b[i] = i;
    *c = *d = 1;
    s.give(b);  // a middle block goes back early, once
    CHECK(g_live.size() == 3 && !g_live.count(b));
    s.give(b);  // (no longer held: nothing happens)
    CHECK(g_frees == 1);
    int16_t* e;
    CHECK(s.take(&e, 5) == 0);
    CHECK(g_live.size() == 4);
  }  // the destructor returns a, c, d, e
  CHECK(g_live.empty() && g_allocs == 5 && g_frees == 5);

  CHECK(early_return(&arena) == -100);
  g_fail_above = ~(size_t)0;
  CHECK(g_live.empty() && g_allocs == 8 && g_frees == 8);

  {  // release, then reuse, then destruction: nothing is given back twice
    ArenaScope s(&arena, nullptr);
    float *p, *q;
    CHECK(s.take(&p, 4) == 0 && s.take(&q, 4) == 0);
    s.release(nullptr);
    CHECK(g_live.empty() && g_frees == 10);
    CHECK(s.take(&p, 4) == 0);
    CHECK(g_live.size() == 1);
  }
  CHECK(g_live.empty() && g_allocs == 11 && g_frees == 11);

  {  // ArenaTmp: one block for a scope; an unused one returns nothing
    ArenaTmp t(&arena, nullptr), unused(&arena, nullptr);
    CHECK(t.take(64) == hipSuccess);
    CHECK(g_live.size() == 1 && g_live[t.as<void>()] == 64);
    t.as<char>()[63] = 1;
  }
  CHECK(g_live.empty() && g_allocs == 12 && g_frees == 12);

  if (g_bad || !g_live.empty() || g_allocs != g_frees) {
    fprintf(stderr, "arena_check FAILED: %d failed checks, %zu live, %d allocs, %d frees\n", g_bad,
            g_live.size(), g_allocs, g_frees);
    return 1;
  }
  printf("arena_check ok: %d blocks, each freed once\n", g_allocs);
  return 0;
}
