// pmx_capi.hip -- host side of the C ABI declared in include/pmx_transfer.h.
//
// The context's life, the new points' upload, the step (pmx_run: the kernels
// of one transfer step sequenced on the context's streams), the downloads, the
// device alloc / free ABI and the host pool.  How a mesh becomes the uploaded
// group -- upload, promotion, adoption, the tet records -- is pmx_background.hip.
#include <hip/hip_runtime.h>
#include <sched.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include <hipcub/hipcub.hpp>
#include "pmx_transfer.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"

// events per recorded step: 0 start, 7 derived data built, 1 hint built,
// 2 volume walk done, 3/5 surface path start (node -> trias fans) / end (side
// stream), 6 joined, 4 end, 8/9 around the point-map's first-incident maps
#define PMX_EV_PER_RUN 10

// errors of the calls that work without a context (per host thread)
static thread_local std::string noctx_err;

// live contexts per device in this process (the fallback grids share the GPU)
static std::atomic<int> &live_contexts(int device) {
  static std::atomic<int> n[64];
  return n[device & 63];
}
void pmx_set_noctx_error(const char *msg) { noctx_err = msg; }

#define CK(x) PMX_CK(pmx_call{ctx}, x)

// pinned staging of at least `bytes`, 25 % slack so that a slowly growing
// ParMmg group does not re-pin every iteration.  Every arena copy is on the
// context's stream and no call waits for its last one (pmx_upload_points
// returns with its coordinates still in flight): the arena is handed out only
// once that stream has drained, so no host write, read or re-pin races a DMA.
char *pmx_hstage(pmx_ctx *ctx, size_t bytes) {
  const pmx_call C{ctx};
  if (!C.hip(hipStreamSynchronize(ctx->stream), "pmx_hstage: stream")) return nullptr;
  const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 20);
  if (!C.hip(ctx->h_stage.grow(bytes, cap), "hipHostMalloc")) return nullptr;
  return ctx->h_stage.p;
}

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

bool pmx_download_qual(pmx_ctx *ctx, const double *dev, int64_t ne, double *qual, int64_t stride) {
  const bool dense = stride == (int64_t)sizeof(double);
  const int4 *htv = (const int4 *)ctx->h_tets.p;
  if (!dense && (!htv || ctx->h_tets.cap < (size_t)(ne + 1) * sizeof(int4))) {
    ctx->err = "qualities: strided output needs the new tets' host copy";
    return false;
  }
  hipStream_t s = ctx->stream;
  char *st = pmx_hstage(ctx, (size_t)(ne + 1) * sizeof(double));
  if (!st) return false;
  const double *h = (const double *)st;
  char *out = (char *)qual;
  const bool nt_q = !dense && ((uintptr_t)out % 8) == 0 && stride % 8 == 0;
  const int64_t nch = std::max<int64_t>(1, std::min<int64_t>(8, (ne + 1) >> 20));
  for (int64_t c = 0; c < nch; c++) {
    const int64_t lo = (ne + 1) * c / nch, hi = (ne + 1) * (c + 1) / nch;
    CK(hipMemcpyAsync(st + lo * 8, dev + lo, (size_t)(hi - lo) * 8, hipMemcpyDeviceToHost, s));
    CK(hipEventRecord(ctx->ev_dl[c], s));
  }
  for (int64_t c = 0; c < nch; c++) {
    const int64_t lo = (ne + 1) * c / nch, hi = (ne + 1) * (c + 1) / nch;
    CK(hipEventSynchronize(ctx->ev_dl[c]));
    if (dense) {
      par_for(lo, hi, [&](int64_t k0, int64_t k1) { memcpy(qual + k0, h + k0, (size_t)(k1 - k0) * 8); });
    } else if (nt_q) {
      // streaming 8-B stores into the records (8-B aligned field and stride):
      // no read for ownership of the caller's record lines
      par_for(std::max<int64_t>(lo, 1), hi, [&](int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; k++)
          if (htv[k].x) {
            long long bits;
            memcpy(&bits, &h[k], sizeof bits);
            __builtin_nontemporal_store(bits, (long long *)(out + k * stride));
          }
        std::atomic_thread_fence(std::memory_order_seq_cst);
      });
    } else {
      par_for(std::max<int64_t>(lo, 1), hi, [&](int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; k++)
          if (htv[k].x) memcpy(out + k * stride, &h[k], sizeof(double));   // any record alignment
      });
    }
  }
  if (dense) qual[0] = 0.0;
  return true;
}

// the pinned copy of the new tets, ne + 1 records
int4 *pmx_ctx::grow_htets(int64_t ne) {
  const size_t bytes = (size_t)(ne + 1) * sizeof(int4);
  if (h_tets.grow(bytes, bytes) != hipSuccess) {
    err = "pinned staging of the new tets";
    return nullptr;
  }
  return (int4 *)h_tets.p;
}

bool pmx_ctx::check_device_errors() {
  if (!ran || !d_counts.p) return true;
  unsigned e = 0;
  if (hipMemcpy(&e, d_counts.p + PMX_CNT_ERR, sizeof e, hipMemcpyDeviceToHost) != hipSuccess) {
    err = "reading the step's device error word failed";
    return false;
  }
  if (e & PMX_DERR_BARRIER) {
    err = "k_fallback: a grid barrier timed out (workgroups not co-resident); the step's "
          "results are invalid";
    return false;
  }
  return true;
}

extern "C" {

pmx_ctx *pmx_create(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return nullptr;
  if (device < 0) device = 0;
  device %= n;
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  pmx_ctx *ctx = new pmx_ctx();
  ctx->device = device;
  // HIP maps a process's streams onto a few hardware queues (4 by default,
  // GPU_MAX_HW_QUEUES) in creation order: a second context's streams share
  // the first one's queues, and two streams on one queue run one after the
  // other.  Contexts alternate their creation order so that the second one's
  // main and surface streams land on the first one's idle residency (topo)
  // and short-lived orphan-mark (up) queues instead of behind its walk
  // (PMX_interpMetricsAndFields runs two groups' steps side by side).
  static std::atomic<unsigned> n_created{0};
  const bool odd = (n_created.fetch_add(1) & 1u) != 0;
  auto mk = [](hipStream_t *st) { return hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess; };
  bool sok;
  if (!odd)
    sok = mk(&ctx->own) && mk(&ctx->side) && mk(&ctx->up) && mk(&ctx->topo);
  else
    sok = mk(&ctx->topo) && mk(&ctx->up) && mk(&ctx->own) && mk(&ctx->side);
  ctx->stream = ctx->own;
  if (!sok ||
      !ctx->ev_topo.create(false) || !ctx->ev_tets.create(false) ||
      ctx->h_nbad.grow(PMX_H_WORDS * sizeof(unsigned), PMX_H_WORDS * sizeof(unsigned)) != hipSuccess ||
      !pmx_create_events(ctx->ev_dl, false) || !pmx_create_events(ctx->ev_eg, false) ||
      !ctx->ev_fork.create(false) || !ctx->ev_fork2.create(false) || !ctx->ev_join.create(false)) {
    pmx_destroy(ctx);
    return nullptr;
  }
  // the fallback's grid barrier needs every workgroup resident at once: size
  // its grid from the occupancy query, sharing the GPU with every live
  // context of this process (at least two: ParMmg groups of one rank, C4: 2
  // per GPU, PMX_interpMetricsAndFields' peer); re-sized in pmx_run when
  // contexts come and go.  Contexts of other processes on the same GPU are
  // not counted: one rank per GPU is the supported deployment.
  live_contexts(device)++;
  ctx->fallback_share = std::max(2, live_contexts(device).load());
  ctx->fallback_blocks = fallback_coresident_blocks(device, ctx->fallback_share);
  if (ctx->fallback_blocks < 1) {
    pmx_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void pmx_destroy(pmx_ctx *ctx) {
  if (!ctx) return;
  if (ctx->fallback_share > 0) live_contexts(ctx->device)--;
  if (ctx->peer) pmx_destroy(ctx->peer);
  ctx->peer = nullptr;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (ctx->side) hipStreamSynchronize(ctx->side);
  if (ctx->topo) hipStreamSynchronize(ctx->topo);
  if (ctx->up) hipStreamSynchronize(ctx->up);
  if (ctx->side) hipStreamDestroy(ctx->side);
  if (ctx->topo) hipStreamDestroy(ctx->topo);
  if (ctx->up) hipStreamDestroy(ctx->up);
  if (ctx->own) hipStreamDestroy(ctx->own);
  delete ctx;                              // the device current, the streams drained: the members release themselves
}

const char *pmx_last_error(pmx_ctx *ctx) {
  if (ctx) return ctx->err.c_str();
  return noctx_err.empty() ? "null context" : noctx_err.c_str();
}

int pmx_set_stream(pmx_ctx *ctx, void *s) {
  if (!ctx) return 0;
  ctx->stream = s ? (hipStream_t)s : ctx->own;
  return 1;
}

int pmx_synchronize(pmx_ctx *ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  CK(hipStreamSynchronize(ctx->stream));
  return ctx->check_device_errors() ? 1 : 0;
}

int pmx_device_info(pmx_ctx *ctx, char *buf, int buflen) {
  if (!ctx) return 0;
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, ctx->device));
  snprintf(buf, (size_t)buflen, "%s %s CUs=%d HBM=%.1fGB", p.name, p.gcnArchName,
           p.multiProcessorCount, (double)p.totalGlobalMem / 1e9);
  return 1;
}

int pmx_upload_points(pmx_ctx *ctx, const pmx_points_view *pv) {
  if (!ctx) return 0;
  ctx->have_pts = ctx->ran = false;
  ctx->have_ntet = false;                  // the new tets belong to the points
  ctx->have_src = false;                   // and so do the source vertices
  Trace tr("points");
  if (ctx->next_topo) {                     // its buffers are about to be reused
    CK(hipStreamSynchronize(ctx->topo));
    ctx->next_topo = false;
  }
  if (ctx->tets_inflight) {                 // d_ntetv / h_tets are about to be reused
    CK(hipEventSynchronize(ctx->ev_tets));
    ctx->tets_inflight = false;
  }
  ctx->tets_pending = false;
  ctx->orph_marks = false;
  ctx->orph_fixed = true;
  ctx->eager_nch = 0;
  if (!pv) { ctx->err = "pmx_upload_points: null view"; return 0; }
  hipSetDevice(ctx->device);
  const int64_t n = pv->last - pv->first + 1;
  if (n < 0 || n >= (1LL << 31) || pv->first < 0 || (n > 0 && (!pv->c || pv->stride < 24))) {
    ctx->err = "pmx_upload_points: bad range or coordinates";
    return 0;
  }
  if (pv->tetra_v && (pv->ne < 0 || pv->tetra_stride < 16)) {
    ctx->err = "pmx_upload_points: bad new-tet view";
    return 0;
  }
  const size_t nn = (size_t)std::max<int64_t>(n, 1);
  // The host packs and sends only what the device cannot derive -- dense
  // coordinates (24 B), tags (2 B), the new tets (16 B) -- in a pinned
  // staging arena, chunked so that DMA overlaps packing.  The kinds, the
  // per-path lists (order-preserving compaction), the list-ordered volume
  // coordinates and the orphan marks are the step's work (pmx_run), as the
  // vertex loop and its tag dispatch are inside the reference's call
  // (src/interpmesh_pmmg.c:535-560).  The host's tag pass gives the launch
  // sizes (upper bounds: orphans are found on the device).
  const int64_t ntet = pv->tetra_v ? pv->ne : 0;
  const size_t o_x = 0, o_tg = o_x + pmx_call::al256(nn * 3 * sizeof(double)),
               total = o_tg + pmx_call::al256(pv->tag ? nn * 2 : 0);
  CK(hipStreamSynchronize(ctx->stream));   // the arena may still feed an earlier copy
  char *st = pmx_hstage(ctx, total);
  if (!st) return 0;
  double *hx = (double *)(st + o_x);
  uint16_t *htg = (uint16_t *)(st + o_tg);
  const char *pc = (const char *)pv->c;
  const char *tg = (const char *)pv->tag;
  if (!pmx_dgrow(ctx, ctx->d_qxyz, nn * 3) || !pmx_dgrow(ctx, ctx->d_kind, nn) || !pmx_dgrow(ctx, ctx->d_qmark, nn + 64) ||   // + 64: the marks' word-wide flush
      !pmx_dgrow(ctx, ctx->d_nsel, 2) || !pmx_dgrow(ctx, ctx->d_vollist, nn) || !pmx_dgrow(ctx, ctx->d_bdylist, nn) ||
      !pmx_dgrow(ctx, ctx->d_ctile, (size_t)std::max<int64_t>(cls_tiles(n), 1)) ||
      (tg && !pmx_dgrow(ctx, ctx->d_qtag, nn)) || (ntet && !pmx_dgrow(ctx, ctx->d_ntetv, (size_t)(ntet + 1))))
    return 0;
  // coordinates (+ bounding box: a promoted background's hint grid) and tags
  // (+ the per-path upper bounds)
  double qlo[64][3], qhi[64][3];
  int64_t cvol[64], cbdy[64];
  const int C = par_chunks(0, n, [&](int ci, int64_t j0, int64_t j1) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    int64_t nv = 0, nb = 0;
    for (int64_t j = j0; j < j1; j++) {
      const double *c = (const double *)(pc + (pv->first + j) * pv->stride);
      for (int ax = 0; ax < 3; ax++) {
        hx[3 * j + ax] = c[ax];
        lo[ax] = std::min(lo[ax], c[ax]);
        hi[ax] = std::max(hi[ax], c[ax]);
      }
      if (tg) {
        const uint16_t t = *(const uint16_t *)(tg + (pv->first + j) * pv->tag_stride);
        htg[j] = t;
        const bool live = t < PMX_TAG_NUL && !(t & PMX_TAG_REQ);
        nv += (live && !(t & PMX_TAG_BDY)) ? 1 : 0;
        nb += (live && (t & PMX_TAG_BDY)) ? 1 : 0;
      }
    }
    for (int ax = 0; ax < 3; ax++) { qlo[ci][ax] = lo[ax]; qhi[ci][ax] = hi[ax]; }
    cvol[ci] = tg ? nv : j1 - j0;
    cbdy[ci] = nb;
  });
  ctx->nq_vol_ub = ctx->nq_bdy_ub = 0;
  for (int i = 0; i < C; i++) {
    ctx->nq_vol_ub += cvol[i];
    ctx->nq_bdy_ub += cbdy[i];
  }
  for (int ax = 0; ax < 3; ax++) {
    ctx->qlo[ax] = HUGE_VAL;
    ctx->qhi[ax] = -HUGE_VAL;
    for (int i = 0; i < C; i++) {
      ctx->qlo[ax] = std::min(ctx->qlo[ax], qlo[i][ax]);
      ctx->qhi[ax] = std::max(ctx->qhi[ax], qhi[i][ax]);
    }
  }
  if (n) {
    CK(hipMemcpyAsync(ctx->d_qxyz.p, hx, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (tg) CK(hipMemcpyAsync(ctx->d_qtag.p, htg, (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream));
  }
  tr.mark("coords");
  // the new tets are packed and sent by the first step on these points
  // (pack_new_tets): their DMA overlaps the step and the download
  ctx->tview = *pv;
  ctx->tets_pending = ntet > 0;
  ctx->view_tets = ntet > 0;
  ctx->nq = n;
  if (!pmx_dgrow(ctx, ctx->d_wmask, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_elem, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_status, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_steps, nn)) return 0;
  // points a step never locates (NUL, frozen, orphans) report element 0
  CK(hipMemsetAsync(ctx->d_elem.p, 0, nn * sizeof(int), ctx->stream));
  CK(hipMemsetAsync(ctx->d_status.p, 0, nn * sizeof(int), ctx->stream));
  CK(hipMemsetAsync(ctx->d_steps.p, 0, nn * sizeof(int), ctx->stream));
  if (!pmx_dgrow(ctx, ctx->d_start, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_edge, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_vertex, nn)) return 0;
  // start 0, edge / vertex unset (-1) for every point no step writes
  CK(hipMemsetAsync(ctx->d_start.p, 0, nn * sizeof(int), ctx->stream));
  CK(hipMemsetAsync(ctx->d_edge.p, 0xff, nn * sizeof(int), ctx->stream));
  CK(hipMemsetAsync(ctx->d_vertex.p, 0xff, nn * sizeof(int), ctx->stream));
  if (!pmx_dgrow(ctx, ctx->d_list, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_found, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_bestk, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_best, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_ties, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_counts, 32)) return 0;
  // one record per wave (sized for every point on one path)
  if (!pmx_dgrow(ctx, ctx->d_vstat, (nn + 255) / 256 * 4 + 4)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_bstat, (nn + 255) / 256 * 4 + 4)) return 0;
  // no wait for the copies: the step queues behind them, and the next host
  // use of the arena waits for the stream (pmx_hstage)
  ctx->have_qtag = tg && n;
  ctx->pts_first = pv->first;
  // orphans (points in no valid new tet) are known once the tets are packed,
  // after the step: the step locates them too and fix_orphans resets their
  // rows before any consumer reads them (the reference never visits them,
  // src/interpmesh_pmmg.c:535-541)
  ctx->have_pts = true;
  ctx->have_ntet = ntet > 0;
  ctx->n_ntet = ntet;
  return 1;
}

// The new points' source vertices (MMG5_Point.src of a USE_POINTMAP build),
// packed dense in the pinned arena and sent on the context's stream.  Any int
// is accepted: a source outside 1..np of the step's background, or one no
// element holds, starts its walk from element 1 (resolved on the device).
int pmx_upload_point_sources(pmx_ctx *ctx, const int *src, int64_t stride) {
  if (!ctx) return 0;
  if (!ctx->have_pts) { ctx->err = "pmx_upload_point_sources: upload the points first"; return 0; }
  ctx->have_src = false;
  if (!src) return 1;
  if (stride < (int64_t)sizeof(int)) { ctx->err = "pmx_upload_point_sources: bad stride"; return 0; }
  hipSetDevice(ctx->device);
  const int64_t n = ctx->nq;
  if (!pmx_dgrow(ctx, ctx->d_qsrc, (size_t)std::max<int64_t>(n, 1))) return 0;
  if (n) {
    int *h = (int *)pmx_hstage(ctx, (size_t)n * sizeof(int));
    if (!h) return 0;
    const char *ps = (const char *)src;
    const int64_t first = ctx->pts_first;
    par_for(0, n, [&](int64_t j0, int64_t j1) {
      for (int64_t j = j0; j < j1; j++) h[j] = *(const int *)(ps + (first + j) * stride);
    });
    CK(hipMemcpyAsync(ctx->d_qsrc.p, h, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  }
  ctx->have_src = true;
  return 1;
}

// ---- the new tets, after the step (pack_new_tets) ------------------------------

// The points view's new tets (vertex = view index - first + 1), validated and
// packed in chunks into their own pinned staging (the shared arena serves the
// download meanwhile), each chunk's DMA on `up` overlapping the packing of
// the next.  Once they are on the device, a kernel on the same stream marks
// the points of valid tets -- the reference's vertex loop over the new tets
// (src/interpmesh_pmmg.c:535-541) -- so that the points in no valid tet
// (orphans: untouched, the reference never visits them) are known to
// fix_orphans.  With residency the next background's tet records are built
// from them on the topo stream once they have arrived.
bool pmx_ctx::pack_new_tets() {
  pmx_ctx *ctx = this;                     // CK()
  if (!tets_pending) return true;
  tets_pending = false;
  const pmx_points_view *pv = &tview;
  const int64_t n = nq, ntet = pv->ne;
  Trace tr("new tets");
  int4 *htv = grow_htets(ntet);
  if (!htv) return false;
  const char *tc = (const char *)pv->tetra_v;
  bool bad = false;
  htv[0] = make_int4(0, 0, 0, 0);
  const int64_t nch = std::max<int64_t>(1, std::min<int64_t>(8, ntet >> 20));
  for (int64_t c = 0; c < nch; c++) {
    const int64_t lo = (c == 0) ? 0 : 1 + ntet * c / nch, hi = 1 + ntet * (c + 1) / nch;
    par_for(std::max<int64_t>(lo, 1), hi, [&](int64_t k0, int64_t k1) {
      bool b = false;
      for (int64_t k = k0; k < k1; k++) {
        const int *v = (const int *)(tc + k * pv->tetra_stride);
        if (v[0] <= 0) { st4(&htv[k], 0, 0, 0, 0); continue; }   // !MG_EOK
        int w[4];
        for (int l = 0; l < 4; l++) {
          int64_t jj = (int64_t)v[l] - pv->first;
          if (jj < 0 || jj >= n) { b = true; jj = 0; }
          w[l] = (int)(jj + 1);
        }
        st4(&htv[k], w[0], w[1], w[2], w[3]);
      }
      if (b) __atomic_store_n(&bad, true, __ATOMIC_RELAXED);
      std::atomic_thread_fence(std::memory_order_seq_cst);
    });
    if (bad) break;
    CK(hipMemcpyAsync(d_ntetv.p + lo, htv + lo, (size_t)(hi - lo) * sizeof(int4), hipMemcpyHostToDevice, up));
  }
  if (!bad && n > 0) {
    // the orphan marks, on the device once the tets are there (the host's
    // byte stores into a point-sized array cost as much as the packing)
    CK(hipMemsetAsync(d_qmark.p, 0, (size_t)n, up));
    launch_mark_new_tets(d_ntetv.p, ntet, d_qmark.p, n, up);
    CK(hipGetLastError());
    orph_marks = true;
  }
  CK(hipEventRecord(ev_tets, up));
  tets_inflight = true;
  if (bad) {
    err = "pmx_run: new tet vertex outside [first, last] of the points view";
    have_ntet = false;
    return false;
  }
  tr.mark("pack + dma issued");
  // residency: the next background's tet records (face adjacency built on
  // the device) on the topo stream, after the tets' DMA, while the step and
  // the download go on
  if (residency && ntet > 0) {
    CK(hipStreamWaitEvent(topo, ev_tets, 0));
    if (!build_records(d_ntetv.p, nullptr, ntet, n, records_next(), topo)) return false;
    CK(hipEventRecord(ev_topo, topo));
    next_topo = true;
  }
  return true;
}

// the new tets on the device before work on stream s reads them
bool pmx_ctx::ensure_tets(hipStream_t s) {
  pmx_ctx *ctx = this;
  if (tets_pending && !pack_new_tets()) return false;
  if (tets_inflight) CK(hipStreamWaitEvent(s, ev_tets, 0));
  return true;
}

// The last step located every live point; the orphans' rows go back to
// "never visited" -- no written solution bit (a constant-size metric stays:
// MMG3D_Set_constantSize writes every valid point), element / status / steps
// 0 -- on the stream, before any consumer of the results.
bool pmx_ctx::fix_orphans() {
  pmx_ctx *ctx = this;
  if (orph_fixed) return true;
  orph_fixed = true;
  if (!ran || !orph_marks || nq == 0) return true;
  if (tets_inflight) CK(hipStreamWaitEvent(stream, ev_tets, 0));   // the marks are written on `up`
  OrphanRows r{d_wmask.p, d_elem.p, d_status.p, d_steps.p, d_start.p, d_edge.p, d_vertex.p, d_kind.p};
  launch_orphans(d_qmark.p, nq, (uint8_t)last_const_bit, r, stream);
  CK(hipGetLastError());
  return true;
}

// the orphan marks from the device copy of the new tets (d_ntetv), on s
bool pmx_ctx::mark_new_tets(hipStream_t s) {
  pmx_ctx *ctx = this;
  if (nq < 1) return true;
  CK(hipMemsetAsync(d_qmark.p, 0, (size_t)nq, s));
  launch_mark_new_tets(d_ntetv.p, n_ntet, d_qmark.p, nq, s);
  CK(hipGetLastError());
  return true;
}

// ---- the step ---------------------------------------------------------------

static void fill_vol_args(pmx_ctx *ctx, const SolDesc &sd, const pmx_run_opts &opts, VolArgs &A) {
  A.xyz = ctx->d_xyz.p; A.tets = ctx->d_tets.p; A.wrec = ctx->d_wrec.p; A.sol = ctx->d_sol.p; A.sd = sd;
  A.q = ctx->d_qxyz.p; A.kind = ctx->d_kind.p; A.nq = ctx->nq; A.ne = ctx->ne;
  A.grid = ctx->d_grid.p; A.g = ctx->grid;
  A.out = ctx->d_out.p; A.wmask = ctx->d_wmask.p;
  A.elem = ctx->d_elem.p; A.status = ctx->d_status.p; A.steps = ctx->d_steps.p;
  A.start = ctx->d_start.p;
  A.stuck_list = ctx->d_list.p; A.stuck_count = ctx->d_counts.p;
  A.tie_list = ctx->d_ties.p; A.tie_count = ctx->d_counts.p + 3;
  A.found = ctx->d_found.p; A.bestk = ctx->d_bestk.p; A.best = ctx->d_best.p;
  A.list = ctx->d_vollist.p; A.nlist = ctx->nq_vol_ub; A.nlist_dev = ctx->d_nsel.p; A.wstats = ctx->d_vstat.p;
  A.max_walk = opts.max_walk > 0 ? opts.max_walk : 512;
  A.const_bit = sd.metric_const ? (1u << sd.imet) : 0u;
  A.inline_ties = (opts.flags & PMX_RUN_NO_INLINE_TIES) ? 0 : 1;
  A.ref_walk = (opts.flags & PMX_RUN_REFERENCE_WALK) ? 1 : 0;
  A.rec_start = (opts.flags & PMX_RUN_RECORD_STARTS) ? 1 : 0;
  A.exp = (opts.flags >> PMX_RUN_EXP_SHIFT) & 0xff;
  // the compact records resolve a far neighbour field when a walk crosses it
  // (a dependent read of the 32-B record); with many such tets the walk on
  // the 32-B records is faster (r05, C3: lex 0 % of the tets, compact 2 %
  // faster; 9 %, 32-B 1.5 % faster; appended 41 %, 32-B 5.5 % faster --
  // DESIGN.md section 7).  exp 18: compact records always
  if (!ctx->compact_recs ||
      (A.exp != 18 && (uint64_t)ctx->h_nbad.p[PMX_H_FAR] * PMX_WREC_FAR_DIV > (uint64_t)std::max<int64_t>(ctx->ne, 1)))
    A.wrec = nullptr;
  A.far = ctx->h_nbad.p[PMX_H_FAR] > 0 ? 1 : 0;
  // point-map starts: no grid; the walks' PM instantiations read the start
  // elements the classification resolved, passed in its place
  if (opts.flags & PMX_RUN_POINTMAP) A.grid = ctx->d_pstart.p;
}

// pmx_run_opts.flags: the public PMX_RUN_* bits, plus the experiment switch
// in bits 16-23 (VolArgs.exp): 6, 17 and 18, which keep the results bit for
// bit.  Anything else is refused, so that a stray bit never changes results
// silently.
static bool run_flags_valid(int flags, std::string *err) {
  const int pub = PMX_RUN_REFERENCE_WALK | PMX_RUN_NO_INLINE_TIES | PMX_RUN_RECORD_STARTS |
                  PMX_RUN_SERIAL_SURFACE | PMX_RUN_FRESH_BACKGROUND | PMX_RUN_DEBUG_BARRIER_TIMEOUT |
                  PMX_RUN_EAGER_DOWNLOAD | PMX_RUN_SEQUENTIAL_SURFACE | PMX_RUN_SEQUENTIAL_VOLUME |
                  PMX_RUN_POINTMAP;
  if (flags & ~(pub | (0xff << PMX_RUN_EXP_SHIFT))) {
    *err = "pmx_run: unknown flag bits";
    return false;
  }
  const int e = (flags >> PMX_RUN_EXP_SHIFT) & 0xff;
  if (e != 0 && e != 6 && e != 17 && e != 18) {
    *err = "pmx_run: unknown experiment switch";
    return false;
  }
  return true;
}

int pmx_run(pmx_ctx *ctx, const pmx_run_opts *o) {
  if (!ctx) return 0;
  ctx->ran = false;
  ctx->eager_nch = 0;
  if (!ctx->have_bg || !ctx->have_pts) { ctx->err = "pmx_run: upload background and points first"; return 0; }
  hipSetDevice(ctx->device);
  pmx_run_opts opts{};
  if (o) opts = *o;
  if (opts.hint_stride < 0 || opts.max_walk < 0) { ctx->err = "pmx_run: bad options"; return 0; }
  if (!run_flags_valid(opts.flags, &ctx->err)) return 0;
  // point-map starts (the reference's USE_POINTMAP): every walk from its
  // point's source vertex.  The sequential modes' speculate-and-replay is
  // built on carried starts: refused together
  const bool pm = (opts.flags & PMX_RUN_POINTMAP) != 0;
  if (pm && (opts.flags & (PMX_RUN_SEQUENTIAL_SURFACE | PMX_RUN_SEQUENTIAL_VOLUME))) {
    ctx->err = "pmx_run: PMX_RUN_POINTMAP cannot be combined with PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME";
    return 0;
  }
  if (pm && !ctx->have_src) {
    ctx->err = "pmx_run: PMX_RUN_POINTMAP needs the sources of the current points (pmx_upload_point_sources)";
    return 0;
  }
  const int64_t n = ctx->nq;
  if (pm && (!pmx_dgrow(ctx, ctx->d_pstart, (size_t)std::max<int64_t>(2 * n, 1)) ||
             !pmx_dgrow(ctx, ctx->d_pmap, (size_t)(2 * (ctx->np + 1))) || !pmx_dgrow(ctx, ctx->d_pmcnt, 2)))
    return 0;
  const int S = ctx->sd.S;
  if (!pmx_dgrow(ctx, ctx->d_out, (size_t)std::max<int64_t>(n * S, 1))) return 0;
  SolDesc sd = ctx->sd;
  sd.metric_const = (opts.hsiz > 0.0 && sd.imet >= 0) ? 1 : 0;

  DevEvent *ev = nullptr;
  if (opts.timing && !(ev = ctx->next_event_slot())) return 0;

  hipStream_t st = ctx->stream;
  // everything below is one iteration's device work on the uploaded raw
  // arrays: the per-background derived data (with PMX_RUN_FRESH_BACKGROUND,
  // or after an upload), the points' classification and compaction, the
  // node -> trias CSR (surface points only), hint grids, walks, fallback.
  // FRESH also redoes every device pass of the uploads (rederive: records,
  // samples, face matching; the fan check; the orphan marks of the new
  // tets): the step is then what a ParMmg iteration costs the device.
  const bool fresh = (opts.flags & PMX_RUN_FRESH_BACKGROUND) != 0;
  const bool derive = !ctx->have_derived || fresh;
  const bool csr = ctx->nq_bdy_ub > 0 && (!ctx->have_csr || fresh);
  // the orphan marks inside the step (FRESH with new tets): the new tets'
  // DMA must have landed (a pending points view is packed now)
  const bool marks = fresh && ctx->have_ntet && n > 0;
  if (marks && !ctx->ensure_tets(st)) return 0;
  if (ev) CK(hipEventRecord(ev[0], st));
  // one prologue kernel zeroes the write masks, the counters and the hint grid
  ZeroRanges z{};
  z.add(ctx->d_wmask.p, n);
  z.add(ctx->d_counts.p, 32 * sizeof(unsigned));
  if (!pm) z.add(ctx->d_grid.p, ctx->gcells * (int64_t)sizeof(int));
  launch_prologue(z, st);
  // the node -> trias fans (PMMG_precompute_nodeTrias, surface points only)
  // on the side stream from the start of the step: a small radix sort that
  // overlaps the derived data, the classification and the hint build
  const bool bdy = ctx->nq_bdy_ub > 0;
  const bool serial = (opts.flags & PMX_RUN_SERIAL_SURFACE) != 0;
  // (r03: the surface stream at the highest priority measured the same,
  // C3 2.093 vs 2.095 ms, profiles/r03_c3_sweep_surface_priority.log)
  hipStream_t side = ctx->side;
  hipStream_t ss = serial ? st : side;
  if (bdy && !serial) {
    CK(hipEventRecord(ctx->ev_fork, st));
    CK(hipStreamWaitEvent(side, ctx->ev_fork, 0));
  }
  // (on the side stream only once it has been forked from the main one: an
  // unforked side stream's event could precede ev[0])
  if (ev) CK(hipEventRecord(ev[3], bdy ? ss : st));
  if (bdy && csr) {
    if (!ctx->build_node_trias(ss, fresh)) return 0;
    ctx->have_csr = true;
  }
  // the orphan marks on `up`, beside the derived data and the hint build
  // (the classification waits for them)
  if (marks) {
    CK(hipEventRecord(ctx->ev_fork, st));
    CK(hipStreamWaitEvent(ctx->up, ctx->ev_fork, 0));
    if (!ctx->mark_new_tets(ctx->up)) return 0;
    CK(hipEventRecord(ctx->ev_tets, ctx->up));
    ctx->tets_inflight = true;
  }
  if (derive) {
    if (bdy && !serial) {
      // the tria normals only feed the surface path: on its stream (r05:
      // the main stream's derived-data pass is the vertices alone)
      launch_bg_derive(ctx->d_xyz.p, ctx->np, ctx->grid, ctx->d_xyzq.p, ctx->d_tris.p, 0, ctx->d_trn.p, st);
      launch_bg_derive(ctx->d_xyz.p, 0, ctx->grid, ctx->d_xyzq.p, ctx->d_tris.p, ctx->nt, ctx->d_trn.p, side);
    } else {
      launch_bg_derive(ctx->d_xyz.p, ctx->np, ctx->grid, ctx->d_xyzq.p, ctx->d_tris.p, ctx->nt,
                       ctx->d_trn.p, st);
    }
    ctx->have_derived = true;
  }
  if (fresh && !ctx->rederive(st)) return 0;
  if (ev) CK(hipEventRecord(ev[7], st));
  // the first-incident-element maps: derived background data like the tria
  // normals, after the records a FRESH step rebuilt, only for a flagged step
  if (ev) CK(hipEventRecord(ev[8], st));
  if (pm && (!ctx->have_pmap || fresh)) {
    launch_pmap_build(ctx->d_tets.p, ctx->ne, ctx->d_tris.p, ctx->nt, ctx->np, ctx->d_pmap.p, ctx->d_pmcnt.p, st);
    ctx->have_pmap = true;
  }
  if (ev) CK(hipEventRecord(ev[9], st));
  // with the marks in the step, the hint build (which does not depend on the
  // points) goes ahead of the classification, beside the marks
  const int stride = opts.hint_stride > 0 ? opts.hint_stride : PMX_HINT_STRIDE;
  const bool packed = stride == PMX_HINT_STRIDE;
  bool any_interp = false;
  for (int s = 0; s < sd.nsol; s++)
    if (!(s == sd.imet && sd.metric_const)) any_interp = true;
  GridDesc g_hint = ctx->grid;
  auto hint_build = [&]() {
    if (pm) return;                          // no grid: the starts come with the classification
    launch_hint_build(packed ? ctx->d_tets_s.p : nullptr,
                      packed && ctx->samples_sorted ? ctx->d_tets_sk.p : nullptr, ctx->d_tets.p, ctx->ne,
                      stride, ctx->d_grid.p, g_hint, ctx->d_xyzq.p, st,
                      packed && ctx->samples_owner ? ctx->nsamp : -1);
  };
  const bool hint_first = marks && any_interp;
  if (hint_first) hint_build();
  if (marks) CK(hipStreamWaitEvent(st, ctx->ev_tets, 0));
  if (!ctx->classify(st, marks, pm)) return 0;
  if (sd.metric_const)
    launch_const_metric(ctx->d_kind.p, n, ctx->d_out.p, S, sd.off[sd.imet], sd.size[sd.imet],
                        opts.hsiz, ctx->d_wmask.p, sd.imet, st);
  // reference early exit (src/interpmesh_pmmg.c:508-512): nothing to locate
  if (!any_interp && bdy && !serial) {
    CK(hipEventRecord(ctx->ev_join, side));
    CK(hipStreamWaitEvent(st, ctx->ev_join, 0));
  }
  if (any_interp) {
    VolArgs A{};
    fill_vol_args(ctx, sd, opts, A);
    // the surface path on the side stream as soon as the points are
    // classified, latency-bound beside the hint build and the volume walk
    // (r03 A/B, profiles/r03_c{2,3,4}_sweep_surface_fork.log: C2 step 0.346 ->
    // 0.338 ms, C3 / C4 within 0.1 %)
    if (bdy && !serial) {
      CK(hipEventRecord(ctx->ev_fork2, st));
      CK(hipStreamWaitEvent(side, ctx->ev_fork2, 0));
      if (!ctx->launch_bdy(A, side, pm)) return 0;
      if (ev) CK(hipEventRecord(ev[5], side));
      CK(hipEventRecord(ctx->ev_join, side));
    }
    if (!hint_first) hint_build();
    if (ev) CK(hipEventRecord(ev[1], st));
    if (ctx->nq_vol_ub) launch_walk(A, st, pm);
    if (ev) CK(hipEventRecord(ev[2], st));
    if (bdy && !serial) {
      CK(hipStreamWaitEvent(st, ctx->ev_join, 0));     // surface path done
    } else if (bdy) {
      if (!ctx->launch_bdy(A, st, pm)) return 0;
      if (ev) CK(hipEventRecord(ev[5], st));
    } else if (ev) {
      CK(hipEventRecord(ev[5], st));
    }
    if (ev) CK(hipEventRecord(ev[6], st));
    ExhArgs E{};
    E.xyz = ctx->d_xyz.p; E.tets = ctx->d_tets.p; E.ne = ctx->ne; E.q = ctx->d_qxyz.p;
    E.list = ctx->d_list.p; E.count = ctx->d_counts.p; E.found = ctx->d_found.p;
    E.best = ctx->d_best.p; E.bestk = ctx->d_bestk.p;
    E.spin_limit = (opts.flags & PMX_RUN_DEBUG_BARRIER_TIMEOUT) ? 0L : (1L << 26);
    const int share = std::max(2, live_contexts(ctx->device).load());
    if (share != ctx->fallback_share) {
      const int fb = fallback_coresident_blocks(ctx->device, share);
      if (fb < 1) { ctx->err = "pmx_run: occupancy query failed"; return 0; }
      ctx->fallback_blocks = fb;
      ctx->fallback_share = share;
    }
    if (ctx->nq_vol_ub) launch_exhaustive(E, A, ctx->fallback_blocks, st);
    // the reference's sequential semantics, after every default result
    ctx->seq_stats_n = -1;
    const bool sq_s = bdy && (opts.flags & PMX_RUN_SEQUENTIAL_SURFACE);
    const bool sq_v = ctx->nq_vol_ub > 0 && (opts.flags & PMX_RUN_SEQUENTIAL_VOLUME);
    if (opts.flags & (PMX_RUN_SEQUENTIAL_SURFACE | PMX_RUN_SEQUENTIAL_VOLUME)) {
      if (!ctx->seq_replay(A, st, sq_s, sq_v)) return 0;
      ctx->seq_stats_n = 1;
    }
    if (ev) CK(hipEventRecord(ev[4], st));
  } else if (ev) {
    for (int k = 1; k < PMX_EV_PER_RUN; k++)
      if (k != 7 && k != 3 && k != 8 && k != 9) CK(hipEventRecord(ev[k], st));
  }
  CK(hipGetLastError());
  // the step located every live point: the orphans' rows are reset by the
  // first consumer of these results (fix_orphans); the new tets are packed
  // and sent now, while the device runs the step
  ctx->last_const_bit = sd.metric_const ? (1u << sd.imet) : 0u;
  // with the marks in the step, the orphans were never located (KIND_ORPH):
  // nothing to reset
  ctx->orph_fixed = marks;
  if (marks) ctx->orph_marks = true;
  ctx->out_S = S;
  ctx->out_n = n;
  ctx->located = any_interp;
  if ((opts.flags & PMX_RUN_EAGER_DOWNLOAD) && !ctx->eager_download()) return 0;
  if (ctx->tets_pending && !ctx->pack_new_tets()) return 0;
  ctx->ran = true;
  return 1;
}

// The fields and write masks of the step just enqueued, down into h_out (its
// own pinned buffer: the arena stays free for the calls in between) in chunks
// on the step's stream.  The orphan reset (fix_orphans, later) changes masks
// only: pmx_download takes them again.
bool pmx_ctx::eager_download() {
  pmx_ctx *ctx = this;
  eager_nch = 0;
  const int64_t n = nq;
  const int S = sd.S;
  if (n == 0 || S == 0) return true;
  const size_t o_wm = pmx_call::al256((size_t)(n * S) * sizeof(double)), bytes = o_wm + pmx_call::al256((size_t)n);
  if (bytes > h_out.cap) {
    CK(hipStreamSynchronize(stream));      // an earlier eager copy may still land in it
    if (h_out.grow(bytes, bytes + bytes / 4) != hipSuccess) {
      err = "pmx_run: pinned staging of the eager download";
      return false;
    }
  }
  const int nch = (int)std::max<int64_t>(1, std::min<int64_t>(4, (n * S) >> 21));
  for (int c = 0; c < nch; c++) {
    const int64_t lo = n * c / nch, hi = n * (c + 1) / nch;
    CK(hipMemcpyAsync(h_out.p + (size_t)(lo * S) * sizeof(double), d_out.p + lo * S,
                      (size_t)((hi - lo) * S) * sizeof(double), hipMemcpyDeviceToHost, stream));
    CK(hipMemcpyAsync(h_out.p + o_wm + lo, d_wmask.p + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, stream));
    CK(hipEventRecord(ev_eg[c], stream));
  }
  eager_nch = nch;
  return true;
}

// results of the last step, consistent with the current uploads
static bool results_ready(pmx_ctx *ctx, const char *who) {
  if (!ctx->ran || !ctx->have_pts || !ctx->have_bg || ctx->out_n != ctx->nq || ctx->out_S != ctx->sd.S) {
    ctx->err = std::string(who) + ": no step has run on the current uploads";
    return false;
  }
  return true;
}

// The step's rows [i0, i1) of the packed fields h (S doubles per point) into
// the caller's per-solution arrays where the write mask has the solution's
// bit.  In blocks of 1024 points, so that every solution reads a block of h
// from cache (solution by solution over the whole range read h once per
// solution).
static void scatter_rows(const pmx_ctx *ctx, const pmx_sol_view *new_sols, const double *h, const uint8_t *wm,
                         int64_t i0, int64_t i1) {
  const int S = ctx->sd.S;
  // streaming 8-B stores (no read for ownership of the caller's lines; the
  // arrays are far larger than the caches anyway)
  for (int64_t b0 = i0; b0 < i1; b0 += 1024) {
    const int64_t b1 = std::min(i1, b0 + 1024);
    for (int s = 0; s < ctx->sd.nsol; s++) {
      double *dst = new_sols[s].m;
      if (!dst) continue;
      const int sz = ctx->sd.size[s], off = ctx->sd.off[s];
      const unsigned bit = 1u << s;
      for (int64_t i = b0; i < b1; i++) {
        if (!(wm[i] & bit)) continue;
        const double *src = h + i * S + off;
        double *d = dst + i * sz;
        for (int j = 0; j < sz; j++) {
          long long bits;
          memcpy(&bits, &src[j], sizeof bits);
          __builtin_nontemporal_store(bits, (long long *)&d[j]);
        }
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_seq_cst);   // the caller reads them next
}

// pmx_download after a PMX_RUN_EAGER_DOWNLOAD step: the fields are (being)
// copied into h_out; each chunk is scattered once it has landed.  elem /
// status / steps come down as usual (after fix_orphans).
static int download_eager(pmx_ctx *ctx, const pmx_sol_view *new_sols, int *elem, int *status, int *steps) {
  const int64_t n = ctx->nq;
  const int S = ctx->sd.S;
  const double *h = (const double *)ctx->h_out.p;
  const uint8_t *wm = (const uint8_t *)(ctx->h_out.p + pmx_call::al256((size_t)(n * S) * sizeof(double)));
  // the eager copy holds the step's masks; with new tets, the orphan reset
  // (fix_orphans, enqueued by pmx_download after them) changed some: take the
  // masks again (n bytes)
  if (ctx->orph_marks) {
    CK(hipMemcpyAsync(const_cast<uint8_t *>(wm), ctx->d_wmask.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
  }
  const bool want_int = elem || status || steps;
  const size_t o_el = 0, o_st = o_el + pmx_call::al256((size_t)n * sizeof(int)), o_sp = o_st + pmx_call::al256((size_t)n * sizeof(int)),
               total = o_sp + pmx_call::al256((size_t)n * sizeof(int));
  char *st = nullptr;
  if (want_int) {
    st = pmx_hstage(ctx, total);               // waits for the stream: the eager chunks have landed
    if (!st) return 0;
    if (elem) CK(hipMemcpyAsync(st + o_el, ctx->d_elem.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (status) CK(hipMemcpyAsync(st + o_st, ctx->d_status.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (steps) CK(hipMemcpyAsync(st + o_sp, ctx->d_steps.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  }
  const int nch = ctx->eager_nch;
  for (int c = 0; c < nch; c++) {
    const int64_t lo = n * c / nch, hi = n * (c + 1) / nch;
    CK(hipEventSynchronize(ctx->ev_eg[c]));
    par_for(lo, hi, [&](int64_t i0, int64_t i1) { scatter_rows(ctx, new_sols, h, wm, i0, i1); });
  }
  if (want_int) {
    CK(hipStreamSynchronize(ctx->stream));
    if (elem) memcpy(elem, st + o_el, (size_t)n * sizeof(int));
    if (status) memcpy(status, st + o_st, (size_t)n * sizeof(int));
    if (steps) memcpy(steps, st + o_sp, (size_t)n * sizeof(int));
  }
  return 1;
}

// the caller's host arrays must hold the points of the step (npts rows):
// refused before anything is written (r04: an output sized by a wrong count
// was written past on the host)
static bool check_cap(pmx_ctx *ctx, const char *who, int64_t cap, int64_t need) {
  if (cap >= need) return true;
  ctx->err = std::string(who) + ": output capacity " + std::to_string(cap) + " < " + std::to_string(need) +
             " entries needed";
  return false;
}

int pmx_download(pmx_ctx *ctx, const pmx_sol_view *new_sols, int64_t npts_cap, int *elem, int *status,
                 int *steps) {
  if (!ctx) return 0;
  if (!results_ready(ctx, "pmx_download")) return 0;
  if (!check_cap(ctx, "pmx_download", npts_cap, ctx->nq)) return 0;
  hipSetDevice(ctx->device);
  if (!ctx->fix_orphans()) return 0;
  const int64_t n = ctx->nq;
  const int S = ctx->sd.S;
  CK(hipStreamSynchronize(ctx->stream));
  if (!ctx->check_device_errors()) return 0;
  if (n == 0) return 1;   // empty step: nothing to copy
  // every device -> host copy lands in the pinned arena (async DMA, one sync),
  // then the host scatters into the caller's (pageable, strided) arrays
  const bool want_sol = new_sols && S > 0;
  if (want_sol && ctx->eager_nch > 0) return download_eager(ctx, new_sols, elem, status, steps);
  const size_t o_out = 0, o_wm = o_out + pmx_call::al256(want_sol ? (size_t)(n * S) * sizeof(double) : 0),
               o_el = o_wm + pmx_call::al256(want_sol ? (size_t)n : 0), o_st = o_el + pmx_call::al256((size_t)n * sizeof(int)),
               o_sp = o_st + pmx_call::al256((size_t)n * sizeof(int)), total = o_sp + pmx_call::al256((size_t)n * sizeof(int));
  char *st = pmx_hstage(ctx, total);
  if (!st) return 0;
  const double *h = (const double *)(st + o_out);
  const uint8_t *wm = (const uint8_t *)(st + o_wm);
  // the fields in chunks: a chunk's scatter into the caller's arrays overlaps
  // the DMA of the next one
  const int64_t nch = want_sol ? std::max<int64_t>(1, std::min<int64_t>(4, (n * S) >> 21)) : 0;
  for (int64_t c = 0; c < nch; c++) {
    const int64_t lo = n * c / nch, hi = n * (c + 1) / nch;
    CK(hipMemcpyAsync(st + o_out + (size_t)(lo * S) * sizeof(double), ctx->d_out.p + lo * S,
                      (size_t)((hi - lo) * S) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(st + o_wm + lo, ctx->d_wmask.p + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipEventRecord(ctx->ev_dl[c], ctx->stream));
  }
  if (elem) CK(hipMemcpyAsync(st + o_el, ctx->d_elem.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (status) CK(hipMemcpyAsync(st + o_st, ctx->d_status.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (steps) CK(hipMemcpyAsync(st + o_sp, ctx->d_steps.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  for (int64_t c = 0; c < nch; c++) {
    const int64_t lo = n * c / nch, hi = n * (c + 1) / nch;
    CK(hipEventSynchronize(ctx->ev_dl[c]));
    par_for(lo, hi, [&](int64_t i0, int64_t i1) { scatter_rows(ctx, new_sols, h, wm, i0, i1); });
  }
  CK(hipStreamSynchronize(ctx->stream));
  if (elem) memcpy(elem, st + o_el, (size_t)n * sizeof(int));
  if (status) memcpy(status, st + o_st, (size_t)n * sizeof(int));
  if (steps) memcpy(steps, st + o_sp, (size_t)n * sizeof(int));
  return 1;
}

int pmx_download_starts(pmx_ctx *ctx, int *start, int64_t cap) {
  if (!ctx || !start) return 0;
  if (!results_ready(ctx, "pmx_download_starts")) return 0;
  if (!check_cap(ctx, "pmx_download_starts", cap, ctx->nq)) return 0;
  hipSetDevice(ctx->device);
  if (!ctx->fix_orphans()) return 0;
  CK(hipStreamSynchronize(ctx->stream));
  if (!ctx->check_device_errors()) return 0;
  if (ctx->nq == 0) return 1;
  CK(hipMemcpy(start, ctx->d_start.p, (size_t)ctx->nq * sizeof(int), hipMemcpyDeviceToHost));
  return 1;
}

int pmx_download_border(pmx_ctx *ctx, int *edge, int *vertex, int64_t cap) {
  if (!ctx) return 0;
  if (!results_ready(ctx, "pmx_download_border")) return 0;
  if (!check_cap(ctx, "pmx_download_border", cap, ctx->nq)) return 0;
  hipSetDevice(ctx->device);
  if (!ctx->fix_orphans()) return 0;
  CK(hipStreamSynchronize(ctx->stream));
  if (!ctx->check_device_errors()) return 0;
  if (ctx->nq == 0) return 1;
  if (edge) CK(hipMemcpy(edge, ctx->d_edge.p, (size_t)ctx->nq * sizeof(int), hipMemcpyDeviceToHost));
  if (vertex) CK(hipMemcpy(vertex, ctx->d_vertex.p, (size_t)ctx->nq * sizeof(int), hipMemcpyDeviceToHost));
  return 1;
}

int pmx_locate_stats_get(pmx_ctx *ctx, pmx_locate_stats *st) {
  if (!ctx || !st) return 0;
  if (!results_ready(ctx, "pmx_locate_stats_get")) return 0;
  hipSetDevice(ctx->device);
  if (!ctx->fix_orphans()) return 0;
  CK(hipStreamSynchronize(ctx->stream));
  if (!ctx->check_device_errors()) return 0;
  // per point, over the points the reference visits (kind VOL / BDY; orphans
  // are KIND_ORPH once fix_orphans has run, NUL / frozen points never
  // located): steps > 0 located by a walk, steps < 0 by an exhaustive scan
  // (the reference's ppt->s sign, src/locate_pmmg.c:840-844), status 0 the
  // closest element (not contained anywhere)
  const int64_t n = ctx->nq;
  std::vector<int> status((size_t)std::max<int64_t>(n, 1)), steps((size_t)std::max<int64_t>(n, 1));
  std::vector<int8_t> kind((size_t)std::max<int64_t>(n, 1));
  if (n) {
    CK(hipMemcpy(status.data(), ctx->d_status.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CK(hipMemcpy(steps.data(), ctx->d_steps.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CK(hipMemcpy(kind.data(), ctx->d_kind.p, (size_t)n, hipMemcpyDeviceToHost));
  }
  // PMMG_locate_postprocessing (src/locate_pmmg.c:995-1028): |steps| of every
  // visited point, the exhaustive ones (steps < 0) included, min / max / mean
  memset(st, 0, sizeof *st);
  int64_t located = 0, sum = 0, mx = 0, mn = ctx->ne;
  for (int64_t i = 0; i < n; i++) {
    const int8_t k = kind[(size_t)i];
    if (k != KIND_VOL && k != KIND_BDY) continue;
    (k == KIND_VOL ? st->nvol : st->nbdy)++;
    int64_t s = steps[(size_t)i];
    if (s < 0) {
      st->nexhaust++;
      s = -s;
    }
    if (status[(size_t)i] == 0) st->nclosest++;
    located++;
    sum += s;
    mx = std::max<int64_t>(mx, s);
    mn = std::min<int64_t>(mn, s);
  }
  st->stepmax = mx;
  st->stepmin = mn;
  st->stepav = located ? (double)sum / (double)located : 0.0;
  return 1;
}

int pmx_locate_wave_stats(pmx_ctx *ctx, int path, pmx_wave_stats *st) {
  if (!ctx || !st || (path != 0 && path != 1)) {
    if (ctx) ctx->err = "pmx_locate_wave_stats: bad arguments";
    return 0;
  }
  if (!results_ready(ctx, "pmx_locate_wave_stats")) return 0;
  if (!ctx->fix_orphans()) return 0;
  int nsel[2] = {0, 0};
  CK(hipStreamSynchronize(ctx->stream));
  if (!ctx->check_device_errors()) return 0;
  if (ctx->nq) CK(hipMemcpy(nsel, ctx->d_nsel.p, sizeof nsel, hipMemcpyDeviceToHost));
  memset(st, 0, sizeof *st);
  const int64_t npath = nsel[path];
  if (!npath) return 1;
  std::vector<uint4> w((size_t)((npath + 255) / 256 * 4));
  CK(hipMemcpy(w.data(), path ? ctx->d_bstat.p : ctx->d_vstat.p, w.size() * sizeof(uint4),
               hipMemcpyDeviceToHost));
  for (const uint4 &r : w) {
    if (!r.x) continue;
    st->waves++;
    st->located += r.x;
    st->step_sum += r.y;
    st->lane_steps += 64 * (int64_t)r.z;
    st->wave_max_hist[std::min<unsigned>(r.z, 15u)]++;
  }
  return 1;
}

int pmx_seq_surface_stats(pmx_ctx *ctx, int64_t *nseq, int64_t *nreplay) {
  if (!ctx || !nseq || !nreplay) return 0;
  if (ctx->seq_stats_n < 0 || !ctx->ran) {
    ctx->err = "pmx_seq_surface_stats: the last step did not run PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME";
    return 0;
  }
  *nseq = ctx->seq_stats[1];
  *nreplay = ctx->seq_stats[0];
  return 1;
}

int pmx_seq_volume_stats(pmx_ctx *ctx, int64_t *nseq, int64_t *nreplay) {
  if (!ctx || !nseq || !nreplay) return 0;
  if (ctx->seq_stats_n < 0 || !ctx->ran) {
    ctx->err = "pmx_seq_volume_stats: the last step did not run PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME";
    return 0;
  }
  *nseq = ctx->seq_stats[3];
  *nreplay = ctx->seq_stats[2];
  return 1;
}

int pmx_step_ready(pmx_ctx *ctx) {
  return ctx && ctx->ran && ctx->have_pts && ctx->have_bg && ctx->out_n == ctx->nq && ctx->out_S == ctx->sd.S;
}

void *pmx_device_buffer(pmx_ctx *ctx, int which) {
  if (!ctx) return nullptr;
  // the orphan rows reset before a caller chains on the results (enqueued on
  // the context stream, which the caller orders its own work after)
  if (ctx->ran && (which == 0 || which == 1 || which == 2)) {
    hipSetDevice(ctx->device);
    if (!ctx->fix_orphans()) return nullptr;
  }
  switch (which) {
    case 0: return ctx->d_out.p;
    case 1: return ctx->d_elem.p;
    case 2: return ctx->d_status.p;
    default: return nullptr;
  }
}

void *pmx_device_alloc(pmx_ctx *ctx, size_t bytes) {
  if (!ctx) return nullptr;
  hipSetDevice(ctx->device);
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
  if (e != hipSuccess) {
    ctx->err = std::string("pmx_device_alloc: ") + hipGetErrorString(e);
    return nullptr;
  }
  if (hipMemset(p, 0, std::max<size_t>(bytes, 1)) != hipSuccess) {
    hipFree(p);
    ctx->err = "pmx_device_alloc: memset";
    return nullptr;
  }
  return p;
}

int pmx_device_free(pmx_ctx *ctx, void *p) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  return (p == nullptr || hipFree(p) == hipSuccess) ? 1 : 0;
}

int pmx_device_download(pmx_ctx *ctx, void *host, const void *dev, size_t bytes) {
  if (!ctx) return 0;
  if (!host || !dev) { ctx->err = "pmx_device_download: null pointer"; return 0; }
  hipSetDevice(ctx->device);
  CK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return 1;
}

int pmx_device_upload(pmx_ctx *ctx, void *dev, const void *host, size_t bytes) {
  if (!ctx) return 0;
  if (!host || !dev) { ctx->err = "pmx_device_upload: null pointer"; return 0; }
  hipSetDevice(ctx->device);
  CK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return 1;
}

int64_t pmx_debug_hint_grid(pmx_ctx *ctx, int *host, int64_t cap) {
  if (!ctx || !ctx->ran || !host) return 0;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return 0;
  const int64_t n = std::min<int64_t>(cap, ctx->gcells);
  if (hipMemcpy(host, ctx->d_grid.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return ctx->gcells;
}

int64_t pmx_debug_live_allocations(void) { return pmx_live_allocations.load(std::memory_order_relaxed); }

int pmx_pointmap_stats(pmx_ctx *ctx, int64_t atomics[2]) {
  if (!ctx || !atomics) return 0;
  if (!ctx->have_pmap) { ctx->err = "pmx_pointmap_stats: no PMX_RUN_POINTMAP step on this background"; return 0; }
  hipSetDevice(ctx->device);
  CK(hipStreamSynchronize(ctx->stream));
  unsigned c[2] = {0, 0};
  CK(hipMemcpy(c, ctx->d_pmcnt.p, sizeof c, hipMemcpyDeviceToHost));
  atomics[0] = c[0];
  atomics[1] = c[1];
  return 1;
}

int pmx_timing_reset(pmx_ctx *ctx) {
  if (!ctx) return 0;
  ctx->ev_used = 0;
  return 1;
}

double pmx_kernel_ms(pmx_ctx *ctx, int which) {
  if (ctx && which == 7) return pmx_more_kernel_ms(ctx);
  if (ctx && which >= 8 && which <= 11) return pmx_graph_kernel_ms(ctx, which);
  if (ctx && (which == 12 || which == 13)) return pmx_contig_kernel_ms(ctx, which);
  if (ctx && (which == 14 || which == 15)) return pmx_split_kernel_ms(ctx, which);
  if (ctx && which >= 16 && which <= 18) return pmx_merge_kernel_ms(ctx, which);
  if (ctx && (which == 19 || which == 20)) return pmx_moveifc_kernel_ms(ctx, which);
  if (!ctx || ctx->ev_used == 0 || which < 0 || which > 6) return -1.0;
  hipStreamSynchronize(ctx->stream);
  double tot = 0.0;
  for (int r = 0; r < ctx->ev_used; r++) {
    const DevEvent *e = &ctx->events[(size_t)r * PMX_EV_PER_RUN];
    float ms = 0.f;
    // 0 hint (prologue + derived data + hint build), 1 volume walk, 2 surface
    // path, 3 fallback, 4 total, 5 derived data (prologue included), 6 the
    // point-map's first-incident maps
    static const int from[7] = {0, 1, 3, 6, 0, 0, 8}, to[7] = {1, 2, 5, 4, 4, 7, 9};
    hipEventElapsedTime(&ms, e[from[which]], e[to[which]]);
    tot += ms;
  }
  return tot / ctx->ev_used;
}

// ---- device residency across ParMmg iterations --------------------------------
//
// PMMG_update_oldGrps (src/libparmmg1.c:653) makes the group's current mesh --
// the previous iteration's new mesh with its interpolated metric and fields
// -- the next interpolation's background.  The new points, their tags and the
// step's results are already on the device; with the new tets uploaded once
// (pmx_upload_new_tets, also used by pmx_new_mesh_qual) the next background
// needs only its boundary trias from the host.

int pmx_set_residency(pmx_ctx *ctx, int on) {
  if (!ctx) return 0;
  ctx->residency = on != 0;
  return 1;
}

int pmx_upload_new_tets(pmx_ctx *ctx, const int *tetra_v, int64_t tetra_stride, int64_t ne) {
  if (!ctx) return 0;
  if (!ctx->have_pts) { ctx->err = "pmx_upload_new_tets: upload the new points first"; return 0; }
  if (!tetra_v || ne < 1 || tetra_stride < 16 || 4 * ne >= (1LL << 31)) {
    ctx->err = "pmx_upload_new_tets: bad new tets";
    return 0;
  }
  hipSetDevice(ctx->device);
  const int64_t first = ctx->pts_first, n = ctx->nq;
  if (ctx->ran && ctx->view_tets) {
    // the last step took its orphans from the points view's tets (never
    // located, or located and reset): other tets would need another step.
    // The same tets are accepted (their pinned copy, packed by that step, is
    // compared row by row); nothing changes on a refusal.
    if (ctx->tets_inflight) {
      CK(hipEventSynchronize(ctx->ev_tets));
      ctx->tets_inflight = false;
    }
    const int4 *old = (const int4 *)ctx->h_tets.p;
    bool same = old && !ctx->tets_pending && ne == ctx->tview.ne;
    const char *tc0 = (const char *)tetra_v;
    for (int64_t k = 1; same && k <= ne; k++) {
      const int *v = (const int *)(tc0 + k * tetra_stride);
      if (v[0] > 0)
        for (int l = 0; l < 4; l++)
          if ((int64_t)v[l] - first < 0 || (int64_t)v[l] - first >= n) {
            ctx->err = "pmx_upload_new_tets: tet vertex outside the uploaded points";
            return 0;
          }
      const int4 o = old[k];
      same = v[0] <= 0 ? o.x == 0
                       : (o.x == (int)(v[0] - first + 1) && o.y == (int)(v[1] - first + 1) &&
                          o.z == (int)(v[2] - first + 1) && o.w == (int)(v[3] - first + 1));
    }
    if (!same) {
      ctx->err = "pmx_upload_new_tets: the last step took its orphans from the points view's new tets; "
                 "other tets need another pmx_run";
      return 0;
    }
  }
  ctx->have_ntet = false;
  if (ctx->next_topo) {                     // built from other tets: drop it
    CK(hipStreamSynchronize(ctx->topo));
    ctx->next_topo = false;
  }
  ctx->tets_pending = false;                // these tets replace the points view's
  if (ctx->tets_inflight) {
    CK(hipEventSynchronize(ctx->ev_tets));
    ctx->tets_inflight = false;
  }
  // packed into the pinned copy of the new tets (a strided quality output
  // reads their validity there)
  int4 *h = ctx->grow_htets(ne);
  if (!h) return 0;
  h[0] = make_int4(0, 0, 0, 0);
  const char *tc = (const char *)tetra_v;
  bool bad = false;
  // vertices renumbered from the points view (first..last) to 1..n: the
  // numbering of a promoted background
  par_for(1, ne + 1, [&](int64_t k0, int64_t k1) {
    bool b = false;
    for (int64_t k = k0; k < k1; k++) {
      const int *v = (const int *)(tc + k * tetra_stride);
      if (v[0] <= 0) { st4(&h[k], 0, 0, 0, 0); continue; }   // !MG_EOK
      int w[4];
      for (int l = 0; l < 4; l++) {
        const int64_t j = (int64_t)v[l] - first;
        if (j < 0 || j >= n) b = true;
        w[l] = (int)(j + 1);
      }
      st4(&h[k], w[0], w[1], w[2], w[3]);
    }
    if (b) __atomic_store_n(&bad, true, __ATOMIC_RELAXED);
    std::atomic_thread_fence(std::memory_order_seq_cst);
  });
  if (bad) { ctx->err = "pmx_upload_new_tets: tet vertex outside the uploaded points"; return 0; }
  if (!pmx_dgrow(ctx, ctx->d_ntetv, (size_t)(ne + 1))) return 0;
  CK(hipMemcpyAsync(ctx->d_ntetv.p, h, (size_t)(ne + 1) * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
  if (ctx->view_tets && n > 0) {
    // these tets replace the points view's: the reference visits the points
    // of THEIR valid tets (src/interpmesh_pmmg.c:535-541), so the orphan
    // marks come from them (a step already run has its orphan rows reset
    // from these marks by the next consumer of its results)
    CK(hipMemsetAsync(ctx->d_qmark.p, 0, (size_t)n, ctx->stream));
    launch_mark_new_tets(ctx->d_ntetv.p, ne, ctx->d_qmark.p, n, ctx->stream);
    CK(hipGetLastError());
    ctx->orph_marks = true;
    if (ctx->ran) ctx->orph_fixed = false;
  }
  CK(hipStreamSynchronize(ctx->stream));
  ctx->n_ntet = ne;
  ctx->have_ntet = true;
  return 1;
}

}  // extern "C"

// ---- pmx_ctx members ----------------------------------------------------------

// the new points' classification and compaction on stream s (the marks, if
// any, zeroed beforehand)
bool pmx_ctx::classify(hipStream_t s, bool marks, bool pointmap) {
  if (nq < 1) return true;
  const uint16_t *tg = have_qtag ? d_qtag.p : nullptr;
  const uint8_t *mk = marks ? d_qmark.p : nullptr;
  if (pointmap) {
    const PointMapArgs pma{d_qsrc.p, d_pmap.p, d_pmap.p + (np + 1), np, d_pstart.p, d_pstart.p + nq};
    launch_classify_pointmap(tg, mk, nq, d_ctile.p, d_kind.p, d_vollist.p, d_bdylist.p, d_nsel.p, pma, s);
  } else {
    launch_classify(tg, mk, nq, d_ctile.p, d_kind.p, d_vollist.p, d_bdylist.p, d_nsel.p, s);
  }
  if (hipGetLastError() != hipSuccess) {
    err = "classification: launch failed";
    return false;
  }
  return true;
}

DevEvent *pmx_ctx::next_event_slot() {
  size_t need = (size_t)(ev_used + 1) * PMX_EV_PER_RUN;
  if (events.size() < need) events.resize(need);
  DevEvent *r = &events[(size_t)ev_used * PMX_EV_PER_RUN];
  for (int k = 0; k < PMX_EV_PER_RUN; k++)
    if (!r[k].create()) {
      err = "pmx_run: creating the timing events failed";
      return nullptr;
    }
  ev_used++;
  return r;
}

pmx_ctx::~pmx_ctx() {
  pmx_split_free(this);
  pmx_merge_free(this);
  pmx_moveifc_free(this);
}
