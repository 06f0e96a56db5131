// pmx_hostpool.hip -- the host thread pool: every host packing pass of the
// library (gathers / scatters of large AoS arrays) runs on it.  Plain C++17,
// no device code and no HIP header: tests/test_hostpool_sanitizer.py compiles
// this file as -x c++ under the thread sanitizer.
#include <sched.h>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "pmx_hostpool.h"

// The process's CPU share: the CPUs it may run on, capped by a cgroup v2 CPU
// quota (cpu.max "quota period"; a GPU box of this pool: 16 of 256).
static unsigned cpu_share() {
  cpu_set_t set;
  unsigned n = 0;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = (unsigned)CPU_COUNT(&set);
  if (!n) n = std::max(1u, std::thread::hardware_concurrency());
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && period > 0 && strcmp(q, "max") != 0) {
      const long long quota = atoll(q);
      if (quota > 0) n = std::min<unsigned>(n, (unsigned)std::max(1LL, (quota + period - 1) / period));
    }
    fclose(f);
  }
  return n;
}
// host gathers/scatters of large AoS arrays split over the CPU share
// (PMX_HOST_THREADS overrides; at most 32).  Measured on a GPU box (16-CPU
// quota of 256, C3 resident cycle, tools/trace_resident.py): 8 threads 89-95
// ms, 16 threads 67-71 ms, 24 threads (throttled by the quota) 77 ms.
// Ranges below PMX_HOST_THREADS_MIN elements (default 2^18) stay serial.
unsigned pmx_host_threads() {
  static const unsigned T = [] {
    const char *e = getenv("PMX_HOST_THREADS");
    unsigned t = e ? (unsigned)std::max(1, atoi(e)) : cpu_share();
    return std::min(t, 32u);
  }();
  return T;
}
int64_t pmx_host_threads_min() {
  static const int64_t M = [] {
    const char *e = getenv("PMX_HOST_THREADS_MIN");
    return e ? std::max<int64_t>(1, atoll(e)) : (int64_t)(1 << 18);
  }();
  return M;
}

// a persistent pool of pmx_host_threads()-1 workers (thread creation per pass
// cost ~0.1 ms per pass and dominated the chunked copies); the calling thread
// takes part.  One job at a time (a mutex serialises concurrent callers).
namespace {
struct HostPool {
  std::mutex run_m;                      // one job at a time
  std::mutex m;
  std::condition_variable cv, done_cv;
  std::vector<std::thread> th;
  const std::function<void(int)> *job = nullptr;
  int njob = 0;
  std::atomic<int> next{0};
  int active = 0;
  unsigned gen = 0;
  bool stop = false;
  explicit HostPool(unsigned nworkers) {
    for (unsigned i = 0; i < nworkers; i++) th.emplace_back([this] { work(); });
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> g(m);
      stop = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
  void drain(const std::function<void(int)> &f, int n) {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) f(i);
  }
  void work() {
    unsigned seen = 0;
    for (;;) {
      const std::function<void(int)> *f;
      int n;
      {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
        f = job;
        n = njob;
        if (!f) continue;                  // woke after that job had finished
        active++;
      }
      drain(*f, n);
      {
        std::lock_guard<std::mutex> g(m);
        if (--active == 0) done_cv.notify_all();
      }
    }
  }
  void run(const std::function<void(int)> &f, int n) {
    std::lock_guard<std::mutex> r(run_m);
    {
      std::lock_guard<std::mutex> g(m);
      job = &f;
      njob = n;
      next.store(0);
      gen++;
    }
    cv.notify_all();
    drain(f, n);
    std::unique_lock<std::mutex> g(m);
    done_cv.wait(g, [&] { return active == 0 && next.load() >= n; });
    job = nullptr;
  }
};
HostPool &host_pool() {
  static HostPool *p = new HostPool(pmx_host_threads() - 1);   // never destroyed: no exit-time joins
  return *p;
}
}  // namespace
void pmx_host_pool_run(const std::function<void(int)> &job, int n) { host_pool().run(job, n); }

void pmx_par_for(int64_t lo, int64_t hi, const std::function<void(int64_t, int64_t)> &f) {
  par_for(lo, hi, f);
}
