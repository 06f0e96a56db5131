// pmx_hostpool.h -- the host thread pool of the packing passes (plain C++17:
// no HIP header, so that pmx_hostpool.hip also compiles as -x c++ for the
// thread-sanitizer check, tests/c/hostpool_tsan.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>

// the pool's thread count (the process's CPU share, PMX_HOST_THREADS
// overrides, at most 32), the range size below which a pass stays serial
// (PMX_HOST_THREADS_MIN, default 2^18), job(0..n-1) over the workers and the
// caller
unsigned pmx_host_threads();
int64_t pmx_host_threads_min();
void pmx_host_pool_run(const std::function<void(int)> &job, int n);
// f(i0, i1) over [lo, hi) on the host pool
void pmx_par_for(int64_t lo, int64_t hi, const std::function<void(int64_t, int64_t)> &f);
// f(chunk, lo, hi) over C contiguous chunks of [lo, hi); returns C
template <class F> static int par_chunks(int64_t lo, int64_t hi, F f) {
  const int64_t n = hi - lo;
  const int C = (pmx_host_threads() <= 1 || n < pmx_host_threads_min()) ? 1 : (int)pmx_host_threads();
  if (C == 1) { f(0, lo, hi); return 1; }
  const int64_t chunk = (n + C - 1) / C;
  const std::function<void(int)> job = [&](int i) {
    const int64_t a = lo + (int64_t)i * chunk, b = std::min(hi, a + chunk);
    f(i, a, std::max(a, b));
  };
  pmx_host_pool_run(job, C);
  return C;
}
template <class F> static void par_for(int64_t lo, int64_t hi, F f) {
  par_chunks(lo, hi, [&](int, int64_t a, int64_t b) { if (a < b) f(a, b); });
}
