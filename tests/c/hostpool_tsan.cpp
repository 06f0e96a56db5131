// Stand-alone check of the host thread pool (parmmg_amd/csrc/pmx_hostpool.hip,
// compiled as plain C++ under the thread sanitizer by
// tests/test_hostpool_sanitizer.py): every element of a range is visited
// exactly once -- above and below the serial threshold, for an empty range,
// for ranges and job counts smaller than the thread count -- and two caller
// threads may be in the pool at once (PMX_interpMetricsAndFields).  The hit
// counters are plain ints: a range handed out twice is a data race as well as
// a wrong count.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "pmx_hostpool.h"

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "hostpool_tsan.cpp:%d: %s\n", __LINE__, #c);      \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static int expected_chunks(int64_t n) {
  return (pmx_host_threads() <= 1 || n < pmx_host_threads_min()) ? 1 : (int)pmx_host_threads();
}

// par_for and par_chunks over [lo, lo + n)
static void check_range(int64_t lo, int64_t n) {
  std::vector<int> hits((size_t)n, 0);
  par_for(lo, lo + n, [&](int64_t a, int64_t b) {
    CHECK(a < b);
    for (int64_t i = a; i < b; i++) hits[(size_t)(i - lo)]++;
  });
  for (int64_t i = 0; i < n; i++) CHECK(hits[(size_t)i] == 1);

  const int want = expected_chunks(n);
  std::vector<int> seen((size_t)want, 0);
  std::vector<int64_t> len((size_t)want, 0);
  const int C = par_chunks(lo, lo + n, [&](int c, int64_t a, int64_t b) {
    // (an empty chunk may lie past the end of a range shorter than the thread count)
    CHECK(c >= 0 && c < want && a <= b && (a == b || (lo <= a && b <= lo + n)));
    if (c < 0 || c >= want) return;
    seen[(size_t)c]++;
    len[(size_t)c] = b - a;
    for (int64_t i = a; i < b; i++) hits[(size_t)(i - lo)]++;
  });
  CHECK(C == want);
  int64_t total = 0;
  for (int c = 0; c < want; c++) {
    CHECK(seen[(size_t)c] == 1);        // every chunk is reported, an empty one included
    total += len[(size_t)c];
  }
  CHECK(total == n);
  for (int64_t i = 0; i < n; i++) CHECK(hits[(size_t)i] == 2);
}

int main() {
  const int64_t T = pmx_host_threads(), M = pmx_host_threads_min();
  printf("threads %lld, serial below %lld\n", (long long)T, (long long)M);
  // above and below the threshold, sizes that the chunks do not divide
  const int64_t sizes[] = {0, 1, T - 1, T + 1, M - 1, M, M + 1, 4 * M + 3, 100003};
  for (int64_t n : sizes)
    if (n >= 0) {
      check_range(0, n);
      check_range(7, n);
    }
  // the pool itself: no job, fewer jobs than threads, many more
  for (int n : {0, 1, 3, 1000}) {
    std::vector<int> hits((size_t)n, 0);
    const std::function<void(int)> job = [&](int i) { hits[(size_t)i]++; };
    pmx_host_pool_run(job, n);
    for (int i = 0; i < n; i++) CHECK(hits[(size_t)i] == 1);
  }
  // the type-erased entry
  {
    std::vector<int> hits(5000, 0);
    pmx_par_for(0, 5000, [&](int64_t a, int64_t b) {
      for (int64_t i = a; i < b; i++) hits[(size_t)i]++;
    });
    for (int h : hits) CHECK(h == 1);
  }
  // two callers at once, each with its own arrays: the pool takes one job at
  // a time, and neither loses or repeats a chunk
  {
    const int64_t n = 4 * M + 11;
    std::vector<int> hits[2] = {std::vector<int>((size_t)n, 0), std::vector<int>((size_t)n, 0)};
    auto caller = [&](int w) {
      for (int rep = 0; rep < 40; rep++)
        par_for(0, n, [&](int64_t a, int64_t b) {
          for (int64_t i = a; i < b; i++) hits[w][(size_t)i]++;
        });
    };
    std::thread t0(caller, 0), t1(caller, 1);
    t0.join();
    t1.join();
    for (int w = 0; w < 2; w++)
      for (int64_t i = 0; i < n; i++) CHECK(hits[w][(size_t)i] == 40);
  }
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("hostpool tsan ok\n");
  return 0;
}
