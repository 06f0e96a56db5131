// pmx_host.h -- host-side ownership and the call helper (host only).
//
// Every device buffer, pinned buffer and event the library owns is a DevBuf,
// a PinBuf or a DevEvent: a member (or a local) that releases what it holds
// in its destructor.  Nothing is registered anywhere.  None of them may have
// static storage duration: a destructor that runs after the HIP runtime has
// shut down crashes at exit.  pmx_alloc / pmx_free below are the only places
// that allocate or free library-owned memory.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <utility>

struct pmx_ctx;

// live library-owned device and pinned allocations of the process
// (pmx_debug_live_allocations)
inline std::atomic<int64_t> pmx_live_allocations{0};

inline hipError_t pmx_alloc(void **p, size_t bytes, bool pinned) {
  const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
  if (e == hipSuccess) pmx_live_allocations.fetch_add(1, std::memory_order_relaxed);
  else *p = nullptr;
  return e;
}
inline void pmx_free(void *p, bool pinned) {
  if (!p) return;
  if (pinned) hipHostFree(p);
  else hipFree(p);
  pmx_live_allocations.fetch_sub(1, std::memory_order_relaxed);
}

// owning memory block of T: device memory, or pinned host memory
template <class T, bool PINNED> struct OwnBuf {
  T *p = nullptr;
  size_t cap = 0;
  OwnBuf() = default;
  OwnBuf(const OwnBuf &) = delete;
  OwnBuf &operator=(const OwnBuf &) = delete;
  OwnBuf(OwnBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  OwnBuf &operator=(OwnBuf &&o) noexcept {
    if (this != &o) {
      release();
      swap(o);
    }
    return *this;
  }
  ~OwnBuf() { release(); }
  void swap(OwnBuf &o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  friend void swap(OwnBuf &a, OwnBuf &b) noexcept { a.swap(b); }
  void release() {
    pmx_free(p, PINNED);
    p = nullptr;
    cap = 0;
  }
  // grow-only (contents not kept): at least `need`, a new block of `fresh`
  // (device: elements, pinned: bytes); p == nullptr and cap == 0 after a failure
  hipError_t grow(size_t need, size_t fresh) {
    if (need <= cap && p) return hipSuccess;
    release();
    const hipError_t e = pmx_alloc((void **)&p, std::max<size_t>(fresh, 1) * (PINNED ? 1 : sizeof(T)), PINNED);
    if (e == hipSuccess) cap = fresh;
    return e;
  }
};
template <class T> using DevBuf = OwnBuf<T, false>;   // cap in elements (pmx_dgrow)
template <class T> using PinBuf = OwnBuf<T, true>;    // cap in bytes

// owning event, created on first use
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(const DevEvent &) = delete;
  DevEvent &operator=(const DevEvent &) = delete;
  DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent &operator=(DevEvent &&o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~DevEvent() {
    if (e) hipEventDestroy(e);
  }
  bool create(bool timing = true) {
    return e || hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming) == hipSuccess;
  }
  operator hipEvent_t() const { return e; }
};
template <size_t N> inline bool pmx_create_events(DevEvent (&ev)[N], bool timing = true) {
  for (auto &e : ev)
    if (!e.create(timing)) return false;
  return true;
}

inline void pmx_set_error(pmx_ctx *ctx, std::string msg);   // ctx->err (pmx_internal.h)

// grow-only device buffer (contents not kept); false + ctx->err on failure
template <class T> inline bool pmx_dgrow(pmx_ctx *ctx, DevBuf<T> &b, size_t n) {
  const hipError_t e = b.grow(n, n);
  if (e != hipSuccess) pmx_set_error(ctx, std::string("hipMalloc: ") + hipGetErrorString(e));
  return e == hipSuccess;
}

// workgroups of a grid-stride launch over `items` work items, `per` of them
// per workgroup: min(max(ceil(items / per), 1), cap)
inline unsigned pmx_grid(int64_t items, int64_t cap, int64_t per = 256) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>((items + per - 1) / per, 1), cap);
}

// One API call's view of its context: who reports, on which stream.
struct pmx_call {
  pmx_ctx *ctx;
  const char *who = nullptr;
  hipStream_t s = nullptr;

  // "who: what"
  bool fail(const std::string &what) const {
    pmx_set_error(ctx, who ? std::string(who) + ": " + what : what);
    return false;
  }
  bool ok(hipError_t e, const char *what) const { return e == hipSuccess || fail(what); }
  // "who: what: <HIP's error string>"
  bool hip(hipError_t e, const char *what) const {
    return e == hipSuccess || fail(std::string(what) + ": " + hipGetErrorString(e));
  }
  // pmx_dgrow with the caller named: "who: hipMalloc: <HIP's error string>"
  template <class T> bool grow(DevBuf<T> &b, size_t n) const {
    const hipError_t e = b.grow(n, n);
    return e == hipSuccess || hip(e, "hipMalloc");
  }
  bool sync(const char *what) const {
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) return fail(what);
    return true;
  }
  static unsigned blocks(int64_t n) { return (unsigned)std::max<int64_t>((n + 255) / 256, 1); }
  static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
  // n control words down, the stream synchronised
  template <class T> bool read_words(T *dst, const T *src, size_t n, const char *what = "control words") const {
    if (hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(what);
    return true;
  }

  // hipcub on the call's stream: size query, scratch grown, call
  template <class In, class Out>
  bool exclusive_sum(DevBuf<char> &tmp, In in, Out out, int64_t n, const char *what) const {
    size_t b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, in, out, (int)n, s);
    return grow(tmp, b) && ok(hipcub::DeviceScan::ExclusiveSum(tmp.p, b, in, out, (int)n, s), what);
  }
  template <class K, class V>
  bool sort_pairs(DevBuf<char> &tmp, const K *kin, K *kout, const V *vin, V *vout, int64_t n, int bits,
                  const char *what) const {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, kin, kout, vin, vout, (int)n, 0, bits, s);
    return grow(tmp, b) &&
           ok(hipcub::DeviceRadixSort::SortPairs(tmp.p, b, kin, kout, vin, vout, (int)n, 0, bits, s), what);
  }
  template <class In, class Flag, class Out>
  bool select_flagged(DevBuf<char> &tmp, In in, Flag flag, Out out, unsigned *nsel, int64_t n, const char *what) const {
    size_t b = 0;
    (void)hipcub::DeviceSelect::Flagged(nullptr, b, in, flag, out, nsel, (int)n, s);
    return grow(tmp, b) && ok(hipcub::DeviceSelect::Flagged(tmp.p, b, in, flag, out, nsel, (int)n, s), what);
  }
  template <class In, class Out, class Sel>
  bool select_if(DevBuf<char> &tmp, In in, Out out, unsigned *nsel, int64_t n, Sel sel, const char *what) const {
    size_t b = 0;
    (void)hipcub::DeviceSelect::If(nullptr, b, in, out, nsel, (int)n, sel, s);
    return grow(tmp, b) && ok(hipcub::DeviceSelect::If(tmp.p, b, in, out, nsel, (int)n, sel, s), what);
  }
};
// in a function that returns 0 on failure: "who: x: <HIP's error string>"
#define PMX_CK(call, x) do { if (!(call).hip((x), #x)) return 0; } while (0)
