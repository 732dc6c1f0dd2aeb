// iqlhip_staging.h — a block of launch records that exists twice: `pin`, pinned host memory the host writes, and `dev`,
// the device memory one asynchronous copy brings it to — with the event recorded behind that copy and the protocol
// around it: wait_free() before the host rewrites `pin`, upload() after.  No other code touches the event or the
// pending flag.  Sections are appended in order (add), each at the next 256-byte boundary; a Section<T> is the typed
// handle of one, host() / device() its view in either copy, at() in any buffer of the same layout.
// A staging is built in place in its owner and is neither copyable nor movable: alloc() hands the addresses of its own
// members to the OwnedT, which nulls them on rollback and release — a copy would leave those addresses dangling.
// CachedStagingT: the form of the calls whose records mostly repeat (an evaluation loop's): the records are built in a
// host buffer of the same layout and uploaded only when their used prefix differs from the last upload's.
// Api supplies, beyond what OwnedT asks for (iqlhip.hip: the HIP runtime; tools/staging_check.cpp: a stub that logs):
//   stream_t, event_no_timing, copy_to_dev, event_record, event_wait.
#pragma once

#include "iqlhip_owned.h"

template <class T> struct Section { size_t off = 0; };

template <class Api> class StagingT {
 public:
  using err_t = typename Api::err_t;
  using stream_t = typename Api::stream_t;

  char* dev = nullptr;
  char* pin = nullptr;
  size_t bytes = 0;

  StagingT() = default;
  StagingT(const StagingT&) = delete;
  StagingT& operator=(const StagingT&) = delete;

  template <class T> Section<T> add(size_t count) {
    Section<T> s;
    s.off = (bytes + 255) / 256 * 256;
    bytes = s.off + count * sizeof(T);
    return s;
  }
  template <class T> static T* at(char* base, Section<T> s) { return (T*)(base + s.off); }
  template <class T> T* host(Section<T> s) const { return at(pin, s); }
  template <class T> const T* device(Section<T> s) const { return at(dev, s); }

  // The two blocks of the layout so far (the pinned one zeroed: records are uploaded — and compared — whole, padding
  // included) and the upload event; with_event = false: a staging of synchronous calls, free again when they return.
  err_t alloc(OwnedT<Api>& own, bool with_event = true) {
    err_t e = own.dev(&dev, bytes);
    if (e == Api::ok) e = own.pin(&pin, bytes, /*zero=*/true);
    if (e == Api::ok && with_event) e = own.event(&up_, Api::event_no_timing);
    return e;
  }
  bool has_event() const { return up_ != typename Api::event_t{}; }

  // Wait until the previous upload has read `pin` (normally long done: the host builds the next call's records while
  // the GPU runs this one's launches).
  err_t wait_free() {
    if (!pending_) return Api::ok;
    const err_t e = Api::event_wait(up_);
    if (e == Api::ok) pending_ = false;
    return e;
  }
  // The first n bytes to the device, on `st`.
  err_t upload(size_t n, stream_t st) {
    err_t e = Api::copy_to_dev(dev, pin, n, st);
    if (e != Api::ok || !has_event()) return e;
    if ((e = Api::event_record(up_, st)) == Api::ok) pending_ = true;
    return e;
  }

 private:
  typename Api::event_t up_{};      // behind the last upload: it has read `pin`
  bool pending_ = false;
};

template <class Api> class CachedStagingT : public StagingT<Api> {
 public:
  using Base = StagingT<Api>;
  using err_t = typename Api::err_t;

  err_t alloc(OwnedT<Api>& own) {
    const err_t e = Base::alloc(own);
    if (e != Api::ok) return e;
    build_.assign(this->bytes, 0);
    last_.assign(this->bytes, 0);
    last_used_ = 0;      // (no upload yet: the first call's differs)
    return e;
  }
  // A section of the build buffer: where the record builders write — never into `pin`, so they may overlap a pending
  // upload.  Its padding bytes stay zero: equal records compare equal.
  template <class T> T* build(Section<T> s) { return Base::at(build_.data(), s); }
  // Upload the first `used` bytes of the build buffer unless they are what the device already holds.
  err_t upload_if_changed(size_t used, typename Api::stream_t st) {
    if (used == last_used_ && memcmp(build_.data(), last_.data(), used) == 0) return Api::ok;
    err_t e = this->wait_free();
    if (e != Api::ok) return e;
    memcpy(this->pin, build_.data(), used);
    if ((e = this->upload(used, st)) != Api::ok) return e;
    memcpy(last_.data(), build_.data(), used);
    last_used_ = used;
    return e;
  }

 private:
  std::vector<char> build_, last_;
  size_t last_used_ = 0;
};
