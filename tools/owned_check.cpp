// owned_check.cpp — stand-alone host check of OwnedT (csrc/iqlhip_owned.h) through a stub allocator: no GPU, no HIP.
//   c++ -std=c++17 -g -fsanitize=address,undefined -I jsrl-corl_amd/csrc tools/owned_check.cpp -o owned_check && ./owned_check
// For every n: a few allocations, a mark, a series of allocations of which the n-th fails, rollback.  Asserted: what
// was made since the mark is freed exactly once, every pointer stored since the mark is null again, what was made
// before the mark survives untouched, release_all frees the rest newest first, and the live count follows.  The stub
// hands out real heap blocks, so a double free, a missed free or a write through a stale pointer is also an
// AddressSanitizer / LeakSanitizer report.
#include "iqlhip_owned.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

struct StubApi {
  using err_t = int;
  struct Ev { int id; };
  using event_t = Ev*;
  static constexpr err_t ok = 0;
  static inline std::map<void*, int> frees;      // block -> times freed (every block ever handed out has an entry)
  static inline std::vector<void*> free_order;
  static inline int calls = 0, fail_at = -1;     // the fail_at-th allocating call from now fails (-1: none)
  static inline bool fail_fill = false;
  static bool failing() { return fail_at >= 0 && calls++ == fail_at; }
  static err_t make(void** p, size_t n) {
    if (failing()) return 2;
    *p = malloc(n ? n : 1);
    memset(*p, 0xA5, n);
    frees[*p] = 0;
    return ok;
  }
  static err_t drop(void* p) {
    CHECK(frees.count(p) == 1);
    CHECK(frees[p] == 0);      // exactly once
    frees[p] = 1;
    free_order.push_back(p);
    free(p);
    return ok;
  }
  static err_t dev_alloc(void** p, size_t n) { return make(p, n); }
  static err_t dev_fill(void* p, int byte, size_t n) {
    if (fail_fill) return 3;
    memset(p, byte, n);
    return ok;
  }
  static err_t dev_free(void* p) { return drop(p); }
  static err_t pin_alloc(void** p, size_t n) { return make(p, n); }
  static err_t pin_free(void* p) { return drop(p); }
  static err_t event_create(event_t* e, unsigned) { return make((void**)e, sizeof(Ev)); }
  static err_t event_destroy(event_t e) { return drop(e); }
  static void reset() { frees.clear(); free_order.clear(); calls = 0; fail_at = -1; fail_fill = false; }
  static int n_freed() { int k = 0; for (auto& f : frees) k += f.second; return k; }
};
using Owned = OwnedT<StubApi>;

// What a lazily enabled feature does: five allocations of the three kinds, stopping at the first error.
struct Feature { float* a = nullptr; char* b = nullptr; StubApi::event_t ev = nullptr; unsigned* c = nullptr; double* d = nullptr; };
static int enable(Owned& own, Feature& f) {
  int e;
  if ((e = own.dev(&f.a, 64, 0))) return e;
  if ((e = own.pin(&f.b, 32, /*zero=*/true))) return e;
  if ((e = own.event(&f.ev, 0))) return e;
  if ((e = own.dev(&f.c, 16, 0xFF))) return e;
  if ((e = own.dev(&f.d, 128))) return e;
  return 0;
}
static const int kFeatureAllocs = 5;

int main() {
  const int64_t live0 = Owned::live().load();
  for (int n = 0; n <= kFeatureAllocs; ++n) {      // n == kFeatureAllocs: nothing fails
    StubApi::reset();
    {
      Owned own;
      float* base0 = nullptr;
      unsigned char* base1 = nullptr;
      StubApi::event_t base_ev = nullptr;
      CHECK(own.dev(&base0, 40, 0) == 0 && own.pin(&base1, 8, true) == 0 && own.event(&base_ev, 1) == 0);
      CHECK(base0[9] == 0.f && base1[7] == 0 && base_ev != nullptr);
      void* const keep[3] = {base0, base1, base_ev};
      CHECK(Owned::live().load() == live0 + 3);

      const size_t mark = own.mark();
      Feature f;
      StubApi::calls = 0;
      StubApi::fail_at = n < kFeatureAllocs ? n : -1;
      const int rc = enable(own, f);
      StubApi::fail_at = -1;
      if (n < kFeatureAllocs) {
        CHECK(rc == 2);
        CHECK(Owned::live().load() == live0 + 3 + n);      // the n allocations in front of the failing one
        own.rollback(mark);
        CHECK(StubApi::n_freed() == n);                     // each freed (exactly once: drop checks)
        CHECK(!f.a && !f.b && !f.ev && !f.c && !f.d);       // every stored pointer is null again
        // a retry sees "not allocated" and succeeds
        CHECK(enable(own, f) == 0);
      } else {
        CHECK(rc == 0);
        own.rollback(own.mark());                           // an empty rollback frees nothing
        CHECK(StubApi::n_freed() == 0);
      }
      CHECK(f.a && f.b && f.ev && f.c && f.d);
      CHECK(f.a[15] == 0.f && f.b[31] == 0 && f.c[3] == 0xFFFFFFFFu);      // fill bytes and the zeroed pinned block
      CHECK(Owned::live().load() == live0 + 3 + kFeatureAllocs);
      // the allocations in front of the mark survived: same blocks, never freed, still the owner's
      CHECK(base0 == keep[0] && base1 == keep[1] && base_ev == keep[2]);
      for (void* p : keep) CHECK(StubApi::frees[p] == 0);
      base0[9] = 1.f;      // (a freed block would be an AddressSanitizer report here)

      // a fill that fails frees its own block and records nothing
      float* g = nullptr;
      StubApi::fail_fill = true;
      const int before = StubApi::n_freed();
      CHECK(own.dev(&g, 24, 0) == 3 && g == nullptr && StubApi::n_freed() == before + 1);
      StubApi::fail_fill = false;
      CHECK(Owned::live().load() == live0 + 3 + kFeatureAllocs);

      // release_all: the rest, newest first, pointers nulled; a second call (and the destructor) frees nothing more
      void* const newest_first[8] = {f.d, f.c, f.ev, f.b, f.a, base_ev, base1, base0};
      const size_t at = StubApi::free_order.size();
      own.release_all();
      CHECK(StubApi::free_order.size() == at + 8);
      for (int i = 0; i < 8; ++i) CHECK(StubApi::free_order[at + i] == newest_first[i]);
      CHECK(!base0 && !base1 && !base_ev && !f.a && !f.b && !f.ev && !f.c && !f.d);
      own.release_all();
      CHECK(StubApi::free_order.size() == at + 8);
      CHECK(Owned::live().load() == live0);
    }
    for (auto& fr : StubApi::frees) CHECK(fr.second == 1);      // every block ever made: freed, once
    printf("fail at allocation %d of %d: ok (%zu blocks made, %zu freed)\n", n < kFeatureAllocs ? n + 1 : 0, kFeatureAllocs,
           StubApi::frees.size(), StubApi::free_order.size());
  }
  // the destructor releases what is left (the local guard of iqlhip_debug_time_kernel)
  StubApi::reset();
  {
    StubApi::event_t e0 = nullptr, e1 = nullptr;      // (in front of the guard: it nulls them when it goes)
    Owned guard;
    CHECK(guard.event(&e0, 0) == 0 && guard.event(&e1, 0) == 0);
  }
  CHECK(StubApi::n_freed() == 2 && Owned::live().load() == live0);
  printf("owned_check: all checks passed\n");
  return 0;
}
