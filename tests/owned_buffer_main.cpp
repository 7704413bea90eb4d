// The owner of the library's device buffers (grasptrajopt_amd/csrc/gto_owned.h) with a counting fake in place of the
// runtime's free: every allocation is freed exactly once, and never through an owner it was moved out of.
// Built with -fsanitize=address,undefined and run by tests/test_capi_cpu.py; prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

#include "gto_owned.h"

static std::vector<int> g_freed;    // times allocation i was freed
static std::vector<char*> g_block;  // its memory: a real allocation, so that the sanitizer sees a second free or a leak too
static int g_fail_next = 0;         // the status the next free reports

static int fake_free(void* p) {
  for (size_t i = 0; i < g_block.size(); ++i)
    if (g_block[i] == p) {
      if (++g_freed[i] == 1) std::free(p);
      return std::exchange(g_fail_next, 0);
    }
  std::fprintf(stderr, "freed a pointer that was never allocated\n");
  std::abort();
}

using Buf = Owned<fake_free>;

static Buf make(size_t bytes) {
  g_block.push_back(static_cast<char*>(std::malloc(bytes)));
  g_freed.push_back(0);
  return Buf(g_block.back(), bytes);
}

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static int freed(const void* p) {
  for (size_t i = 0; i < g_block.size(); ++i)
    if (g_block[i] == p) return g_freed[i];
  return -1;
}

int main() {
  static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "owners are not copied");
  static_assert(std::is_nothrow_move_constructible<Buf>::value, "a vector of owners moves them when it grows");
  {  // an empty owner frees nothing, as often as it is asked
    Buf e;
    CHECK(!e && e.get() == nullptr && e.bytes() == 0 && e.reset() == 0 && e.reset() == 0);
  }
  {  // move construction: the source is empty and frees nothing
    Buf a = make(16);
    void* p = a.get();
    Buf b(std::move(a));
    CHECK(!a && a.bytes() == 0 && b.get() == p && b.bytes() == 16 && b.as<char>() == p);
    CHECK(a.reset() == 0 && freed(p) == 0);
  }
  {  // move assignment onto a non-empty owner frees what it held, once; self-move keeps it
    Buf a = make(8), b = make(24);
    void *pa = a.get(), *pb = b.get();
    a = std::move(b);
    CHECK(freed(pa) == 1 && freed(pb) == 0 && a.get() == pb && a.bytes() == 24 && !b);
    Buf& self = a;
    a = std::move(self);
    CHECK(a.get() == pb && a.bytes() == 24 && freed(pb) == 0);
    CHECK(a.reset() == 0 && freed(pb) == 1 && !a && a.bytes() == 0);
    CHECK(a.reset() == 0 && freed(pb) == 1);  // reset() twice
  }
  {  // reset() hands the free's status on and empties the owner all the same
    Buf a = make(8);
    void* p = a.get();
    g_fail_next = 7;
    CHECK(a.reset() == 7 && !a && freed(p) == 1 && a.reset() == 0 && freed(p) == 1);
  }
  {  // a vector of owners grows past its capacity; erasing from the middle, as the spare list does
    std::vector<Buf> v;
    std::vector<void*> ps;
    for (int i = 0; i < 100; ++i) {
      v.push_back(make(32 + i));
      ps.push_back(v.back().get());
    }
    for (void* p : ps) CHECK(freed(p) == 0);
    Buf taken = std::move(v[40]);  // the spare whose size matched
    v.erase(v.begin() + 40);
    CHECK(v.size() == 99 && v[40].get() == ps[41] && v[40].bytes() == 32 + 41 && taken.get() == ps[40]);
    for (void* p : ps) CHECK(freed(p) == 0);
    std::vector<Buf> w = std::move(v);  // a scene's owners moving into the table
    v.push_back(make(5));
    v = std::move(w);  // ... and the spares being replaced: what was there is freed
    CHECK(g_freed.back() == 1 && v.size() == 99);
    v.clear();
    for (size_t i = 0; i < ps.size(); ++i) CHECK(freed(ps[i]) == (i == 40 ? 0 : 1));
  }
  for (int n : g_freed) CHECK(n == 1);  // every scope is closed: everything was freed exactly once
  std::puts("ok");
  return 0;
}
