// staging_check.cpp — stand-alone host check of StagingT / CachedStagingT (csrc/iqlhip_staging.h) with OwnedT through a
// stub runtime: no GPU, no HIP.
//   c++ -std=c++17 -g -fsanitize=address,undefined -I jsrl-corl_amd/csrc tools/staging_check.cpp -o staging_check && ./staging_check
// The stub hands out heap blocks, really copies, and logs every copy (source, destination, bytes, stream), every event
// record and every event wait, in order.  Asserted: the section offsets of a layout; upload = the copy, then the event
// record behind it, and a wait_free that waits once and only when an upload is pending; upload_if_changed uploads what
// differs from the last upload inside the used prefix (or a prefix of another length) and nothing else; an n-th
// allocation that fails inside alloc leaves the staging's members null and the owner's count where it was, for every n;
// and release_all nulls the members of a staging allocated in place.  With the sanitizers, a write through a slot that
// no longer exists, a double free or a leak is a report as well.
#include "iqlhip_staging.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

struct StubApi {
  using err_t = int;
  struct Ev { int id; };
  using event_t = Ev*;
  using stream_t = int;
  static constexpr err_t ok = 0;
  static constexpr unsigned event_no_timing = 2;
  enum Op { COPY, RECORD, WAIT };
  struct Entry { Op op; const void* src; void* dst; size_t bytes; stream_t st; event_t ev; };
  static inline std::vector<Entry> log;
  static inline int calls = 0, fail_at = -1;     // the fail_at-th allocating call from now fails (-1: none)
  static inline int blocks = 0;                  // heap blocks out now
  static inline unsigned last_event_flags = 0;
  static err_t make(void** p, size_t n) {
    if (fail_at >= 0 && calls++ == fail_at) return 2;
    *p = malloc(n ? n : 1);
    memset(*p, 0xA5, n);
    ++blocks;
    return ok;
  }
  static err_t drop(void* p) { free(p); --blocks; return ok; }
  static err_t dev_alloc(void** p, size_t n) { return make(p, n); }
  static err_t dev_fill(void* p, int byte, size_t n) { memset(p, byte, n); return ok; }
  static err_t dev_free(void* p) { return drop(p); }
  static err_t pin_alloc(void** p, size_t n) { return make(p, n); }
  static err_t pin_free(void* p) { return drop(p); }
  static err_t event_create(event_t* e, unsigned flags) { last_event_flags = flags; return make((void**)e, sizeof(Ev)); }
  static err_t event_destroy(event_t e) { return drop(e); }
  static err_t copy_to_dev(void* dst, const void* src, size_t n, stream_t st) {
    memcpy(dst, src, n);
    log.push_back(Entry{COPY, src, dst, n, st, nullptr});
    return ok;
  }
  static err_t event_record(event_t e, stream_t st) { log.push_back(Entry{RECORD, nullptr, nullptr, 0, st, e}); return ok; }
  static err_t event_wait(event_t e) { log.push_back(Entry{WAIT, nullptr, nullptr, 0, 0, e}); return ok; }
};
using Owned = OwnedT<StubApi>;
using Staging = StagingT<StubApi>;
using CachedStaging = CachedStagingT<StubApi>;
using Log = StubApi;

static_assert(!std::is_copy_constructible<Staging>::value && !std::is_copy_assignable<Staging>::value, "a staging is not copyable");
static_assert(!std::is_move_constructible<Staging>::value && !std::is_move_assignable<Staging>::value, "a staging is not movable");
static_assert(!std::is_copy_constructible<CachedStaging>::value && !std::is_move_constructible<CachedStaging>::value,
              "nor is its cached form");

struct Odd { char c[13]; };

// What owns a staging in the library: a handle with the owner and the staging in place.
struct Handle {
  Staging stg;      // (in front of the owner: its destructor, which writes the members' slots, runs first)
  Owned own;
  Section<char> a; Section<double> b; Section<Odd> c;
  void lay_out() { a = stg.add<char>(3); b = stg.add<double>(5); c = stg.add<Odd>(7); }
};

static bool is_copy(size_t i, const void* src, void* dst, size_t bytes, int st) {
  const Log::Entry& e = Log::log[i];
  return e.op == Log::COPY && e.src == src && e.dst == dst && e.bytes == bytes && e.st == st;
}

int main() {
  const int64_t live0 = Owned::live().load();
  {      // layout: every section at the next 256-byte boundary, bytes = the end of the last
    Handle h;
    h.lay_out();
    CHECK(h.a.off == 0 && h.b.off == 256 && h.c.off == 512);
    CHECK(h.stg.bytes == 512 + 7 * 13);
    char base[600];
    CHECK((char*)Staging::at(base, h.b) == base + 256);

    // alloc: device block, zeroed pinned block, event without timing — three items of the owner
    CHECK(h.stg.alloc(h.own) == 0);
    CHECK(h.stg.dev && h.stg.pin && h.stg.has_event() && Log::last_event_flags == Log::event_no_timing);
    CHECK(Owned::live().load() == live0 + 3);
    for (size_t i = 0; i < h.stg.bytes; ++i) CHECK(h.stg.pin[i] == 0);
    CHECK((char*)h.stg.host(h.c) == h.stg.pin + 512 && (const char*)h.stg.device(h.c) == h.stg.dev + 512);

    // wait_free with nothing pending: no wait.  upload: the copy, then the record behind it, on the caller's stream.
    CHECK(h.stg.wait_free() == 0 && Log::log.empty());
    h.stg.host(h.b)[4] = 2.5;
    CHECK(h.stg.upload(300, /*stream=*/7) == 0);
    CHECK(Log::log.size() == 2 && is_copy(0, h.stg.pin, h.stg.dev, 300, 7));
    CHECK(Log::log[1].op == Log::RECORD && Log::log[1].st == 7 && Log::log[1].ev != nullptr);
    CHECK(h.stg.device(h.b)[4] == 2.5);
    // pending: wait_free waits once, on the recorded event, and not again
    CHECK(h.stg.wait_free() == 0);
    CHECK(Log::log.size() == 3 && Log::log[2].op == Log::WAIT && Log::log[2].ev == Log::log[1].ev);
    CHECK(h.stg.wait_free() == 0 && Log::log.size() == 3);

    // release_all nulls the staging's own members: they are the slots the owner recorded
    h.own.release_all();
    CHECK(!h.stg.dev && !h.stg.pin && !h.stg.has_event());
    CHECK(Owned::live().load() == live0 && Log::blocks == 0);
  }
  printf("layout, upload, wait_free, release_all: ok\n");

  {      // a staging of synchronous calls: no event, upload is the copy alone and nothing is ever pending
    Handle h;
    h.lay_out();
    Log::log.clear();
    CHECK(h.stg.alloc(h.own, /*with_event=*/false) == 0);
    CHECK(h.stg.dev && h.stg.pin && !h.stg.has_event() && Owned::live().load() == live0 + 2);
    CHECK(h.stg.upload(h.stg.bytes, 1) == 0 && h.stg.wait_free() == 0);
    CHECK(Log::log.size() == 1 && is_copy(0, h.stg.pin, h.stg.dev, h.stg.bytes, 1));
  }
  CHECK(Owned::live().load() == live0 && Log::blocks == 0);      // (the owner's destructor released them)
  printf("no event: ok\n");

  for (int n = 0; n <= 3; ++n) {      // the n-th allocation inside alloc fails (n == 3: none does), all-or-nothing as the library's
    Handle h;
    h.lay_out();
    float* before = nullptr;
    CHECK(h.own.dev(&before, 16, 0) == 0);
    const size_t mark = h.own.mark();
    Log::calls = 0;
    Log::fail_at = n < 3 ? n : -1;
    const int rc = h.stg.alloc(h.own);
    Log::fail_at = -1;
    if (n < 3) {
      CHECK(rc == 2);
      h.own.rollback(mark);
      CHECK(!h.stg.dev && !h.stg.pin && !h.stg.has_event());
      CHECK(Owned::live().load() == live0 + 1 && Log::blocks == 1 && before != nullptr);
      h.stg.bytes = 0;      // a retry lays out again and succeeds
      h.lay_out();
      CHECK(h.stg.bytes == 512 + 7 * 13 && h.stg.alloc(h.own) == 0);
    } else {
      CHECK(rc == 0);
    }
    CHECK(h.stg.dev && h.stg.pin && h.stg.has_event() && Owned::live().load() == live0 + 4);
    h.own.release_all();
    CHECK(!h.stg.dev && !h.stg.pin && !h.stg.has_event() && !before && Log::blocks == 0);
    printf("fail at allocation %d of 3: ok\n", n < 3 ? n + 1 : 0);
  }

  {      // the cached form
    Owned own;
    CachedStaging c;
    const Section<int> s0 = c.add<int>(10);
    const Section<char> s1 = c.add<char>(100);
    CHECK(c.alloc(own) == 0 && Owned::live().load() == live0 + 3);
    Log::log.clear();
    int* rec = c.build(s0);
    char* tail = c.build(s1);
    CHECK((char*)rec != c.pin && rec[9] == 0 && tail[99] == 0);      // the build buffer: its own, zeroed
    const size_t used = s1.off + 40;
    rec[3] = 17; tail[39] = 1;
    // first call: uploads (nothing is pending: no wait) the used prefix, through pin
    CHECK(c.upload_if_changed(used, 5) == 0);
    CHECK(Log::log.size() == 2 && is_copy(0, c.pin, c.dev, used, 5) && Log::log[1].op == Log::RECORD);
    CHECK(c.device(s0)[3] == 17 && c.device(s1)[39] == 1);
    // the same records again: no wait, no copy
    CHECK(c.upload_if_changed(used, 5) == 0 && Log::log.size() == 2);
    // a byte beyond `used` changes: ignored
    tail[40] = 9;
    CHECK(c.upload_if_changed(used, 5) == 0 && Log::log.size() == 2);
    // one byte inside `used` changes: wait for the pending upload, then copy and record
    tail[39] = 2;
    CHECK(c.upload_if_changed(used, 6) == 0);
    CHECK(Log::log.size() == 5 && Log::log[2].op == Log::WAIT && is_copy(3, c.pin, c.dev, used, 6) && Log::log[4].op == Log::RECORD);
    CHECK(c.device(s1)[39] == 2 && c.device(s1)[40] != 9);
    // only `used` changes (same bytes): uploads the new prefix
    CHECK(c.upload_if_changed(used + 1, 6) == 0);
    CHECK(Log::log.size() == 8 && Log::log[5].op == Log::WAIT && is_copy(6, c.pin, c.dev, used + 1, 6) && Log::log[7].op == Log::RECORD);
    CHECK(c.device(s1)[40] == 9);
    CHECK(c.upload_if_changed(used + 1, 6) == 0 && Log::log.size() == 8);
    own.release_all();
    CHECK(!c.dev && !c.pin && !c.has_event());
  }
  CHECK(Owned::live().load() == live0 && Log::blocks == 0);
  printf("upload_if_changed: ok\n");
  printf("staging_check: all checks passed\n");
  return 0;
}
