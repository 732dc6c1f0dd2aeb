// iqlhip_owned.h — the one owner of a context's (or a trainer group's) device buffers, pinned host buffers and events.
// Every allocation goes through dev() / pin() / event(): the call allocates, optionally fills, stores the result
// through the caller's pointer and records it.  release_all() frees what was recorded, newest first; mark() and
// rollback(mark) make a set of allocations all-or-nothing: rollback frees what was made since the mark and nulls the
// pointers it was stored through, so an "already allocated" test on any of them stays truthful.
// Api supplies the allocator (iqlhip.hip: the HIP runtime; tools/owned_check.cpp: a stub that counts and can fail):
//   err_t, event_t, ok, dev_alloc, dev_fill, dev_free, pin_alloc, pin_free, event_create, event_destroy.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

template <class Api> class OwnedT {
 public:
  using err_t = typename Api::err_t;
  using event_t = typename Api::event_t;
  enum { NO_FILL = -1 };

  OwnedT() = default;
  OwnedT(const OwnedT&) = delete;
  OwnedT& operator=(const OwnedT&) = delete;
  ~OwnedT() { release_all(); }

  // Device memory; fill: the byte every byte of it is set to (NO_FILL: left as allocated).
  template <class T> err_t dev(T** p, size_t bytes, int fill = NO_FILL) {
    void* q = nullptr;
    err_t e = Api::dev_alloc(&q, bytes);
    if (e != Api::ok) return e;
    if (fill != NO_FILL && (e = Api::dev_fill(q, fill, bytes)) != Api::ok) {
      (void)Api::dev_free(q);
      return e;
    }
    *p = (T*)q;
    return made(DEV, p, q);
  }
  // Pinned, host-mapped memory.
  template <class T> err_t pin(T** p, size_t bytes, bool zero = false) {
    void* q = nullptr;
    const err_t e = Api::pin_alloc(&q, bytes);
    if (e != Api::ok) return e;
    if (zero) memset(q, 0, bytes);
    *p = (T*)q;
    return made(PIN, p, q);
  }
  err_t event(event_t* ev, unsigned flags) {
    event_t q{};
    const err_t e = Api::event_create(&q, flags);
    if (e != Api::ok) return e;
    *ev = q;
    items_.push_back(Item{EVENT, ev, nullptr, q});
    live().fetch_add(1, std::memory_order_relaxed);
    return Api::ok;
  }

  size_t mark() const { return items_.size(); }
  void rollback(size_t mark) {
    while (items_.size() > mark) {
      const Item it = items_.back();
      items_.pop_back();
      if (it.kind == EVENT) { (void)Api::event_destroy(it.ev); *(event_t*)it.slot = event_t{}; }
      else { (void)(it.kind == DEV ? Api::dev_free(it.mem) : Api::pin_free(it.mem)); *(void**)it.slot = nullptr; }
      live().fetch_sub(1, std::memory_order_relaxed);
    }
  }
  void release_all() { rollback(0); }

  // Buffers and events this process holds in any OwnedT<Api> right now (tests look at its differences).
  static std::atomic<int64_t>& live() {
    static std::atomic<int64_t> n{0};
    return n;
  }

 private:
  enum Kind { DEV, PIN, EVENT };
  struct Item { Kind kind; void* slot; void* mem; event_t ev; };
  err_t made(Kind kind, void* slot, void* mem) {
    items_.push_back(Item{kind, slot, mem, event_t{}});
    live().fetch_add(1, std::memory_order_relaxed);
    return Api::ok;
  }
  std::vector<Item> items_;
};
