// pmx_capi.hip -- host side of the C ABI declared in include/pmx_transfer.h:
// the context's life, the device alloc / free / copy ABI, and the step
// (pmx_run: the kernels of one transfer step sequenced on the context's
// streams, in the phases of struct Step).
//
// k_prologue         the step's first launch: zeroes the write masks, the
//                    counters and the volume hint grid
// k_const_metric     the constant-size metric of every valid point
//
// The rest of the ABI's host side by subject: the new points and the new tets
// are pmx_points.hip, the downloads and the statistics getters
// pmx_results.hip, the host thread pool pmx_hostpool.hip.  How a mesh becomes
// the uploaded group -- upload, promotion, adoption, the tet records -- is
// pmx_background.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <string>
#include <vector>

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

// ---- the context's life -----------------------------------------------------------

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

bool pmx_ctx::check_device_errors() {
  const pmx_call C{this};
  if (!ran || !d_counts.p) return true;
  unsigned e = 0;
  if (!C.ok(hipMemcpy(&e, d_counts.p + PMX_CNT_ERR, sizeof e, hipMemcpyDeviceToHost),
            "reading the step's device error word failed"))
    return false;
  if (e & PMX_DERR_BARRIER)
    return C.fail("k_fallback: a grid barrier timed out (workgroups not co-resident); the step's "
                  "results are invalid");
  return true;
}

pmx_ctx::~pmx_ctx() {
  pmx_split_free(this);
  pmx_merge_free(this);
  pmx_moveifc_free(this);
  pmx_part_drop(this);
}

extern "C" {

// (no context to report to before one exists: the HIP results are compared by hand here)
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
      !ctx->ntets.ev_topo.create(false) || !ctx->ntets.ev.create(false) ||
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
  PMX_CK(pmx_call{ctx}, hipStreamSynchronize(ctx->stream));
  return ctx->check_device_errors() ? 1 : 0;
}

int pmx_device_info(pmx_ctx *ctx, char *buf, int buflen) {
  if (!ctx) return 0;
  hipDeviceProp_t p;
  PMX_CK(pmx_call{ctx}, hipGetDeviceProperties(&p, ctx->device));
  snprintf(buf, (size_t)buflen, "%s %s CUs=%d HBM=%.1fGB", p.name, p.gcnArchName,
           p.multiProcessorCount, (double)p.totalGlobalMem / 1e9);
  return 1;
}

int64_t pmx_debug_live_allocations(void) { return pmx_live_allocations.load(std::memory_order_relaxed); }

// ---- the device-memory ABI --------------------------------------------------------

void *pmx_device_alloc(pmx_ctx *ctx, size_t bytes) {
  if (!ctx) return nullptr;
  const pmx_call C{ctx, "pmx_device_alloc"};
  hipSetDevice(ctx->device);
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
  if (!C.ok(e, hipGetErrorString(e))) return nullptr;
  if (!C.ok(hipMemset(p, 0, std::max<size_t>(bytes, 1)), "memset")) {
    hipFree(p);
    return nullptr;
  }
  return p;
}

// (a failed free reports through the return value alone, as it always has)
int pmx_device_free(pmx_ctx *ctx, void *p) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  return (p == nullptr || hipFree(p) == hipSuccess) ? 1 : 0;
}

int pmx_device_download(pmx_ctx *ctx, void *host, const void *dev, size_t bytes) {
  if (!ctx) return 0;
  const pmx_call C{ctx};
  if (!host || !dev) return C.fail("pmx_device_download: null pointer");
  hipSetDevice(ctx->device);
  PMX_CK(C, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  PMX_CK(C, hipStreamSynchronize(ctx->stream));
  return 1;
}

int pmx_device_upload(pmx_ctx *ctx, void *dev, const void *host, size_t bytes) {
  if (!ctx) return 0;
  const pmx_call C{ctx};
  if (!host || !dev) return C.fail("pmx_device_upload: null pointer");
  hipSetDevice(ctx->device);
  PMX_CK(C, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  PMX_CK(C, hipStreamSynchronize(ctx->stream));
  return 1;
}

}  // extern "C"

// ---- the step ---------------------------------------------------------------

// the step's first launch zeroes up to PMX_ZERO_MAX device ranges
#define PMX_ZERO_MAX 3
struct ZeroRanges {
  void *p[PMX_ZERO_MAX];
  int64_t bytes[PMX_ZERO_MAX];
  int n;
  void add(void *ptr, int64_t b) {
    if (ptr && b > 0) { p[n] = ptr; bytes[n] = b; n++; }
  }
};
// the step's first launch: zero the ranges pmx_run adds -- the write masks,
// the step's counters and the volume hint grid (the orphan marks come from
// the host, the node -> trias counts are zeroed by their own builder)
__global__ __launch_bounds__(256) void k_prologue(ZeroRanges z) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
  for (int r = 0; r < z.n; r++) {
    // hipMalloc'd ranges: 256-B aligned starts
    const int64_t n16 = z.bytes[r] / 16;
    uint4 *q = reinterpret_cast<uint4 *>(z.p[r]);
    for (int64_t i = t; i < n16; i += st) q[i] = make_uint4(0, 0, 0, 0);
    char *c = reinterpret_cast<char *>(z.p[r]);
    for (int64_t i = n16 * 16 + t; i < z.bytes[r]; i += st) c[i] = 0;
  }
}
static void launch_prologue(const ZeroRanges &z, hipStream_t s) {
  int64_t work = 1;
  for (int r = 0; r < z.n; r++) work = std::max<int64_t>(work, z.bytes[r] / 16);
  hipLaunchKernelGGL(k_prologue, dim3(pmx_grid(work, 4096)), dim3(256), 0, s, z);
}

// constant-size metric (MMG3D_Set_constantSize restated): all valid points
__global__ __launch_bounds__(256) void k_const_metric(const int8_t *__restrict__ kind, int64_t nq,
                                                      double *__restrict__ out, int S, int off,
                                                      int size, double hsiz,
                                                      uint8_t *__restrict__ wmask, int imet) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (kind[i] == KIND_NUL) continue;
    double *o = out + i * S + off;
    if (size == 1) {
      o[0] = hsiz;
    } else {
      double v = 1.0 / (hsiz * hsiz);
      o[0] = v; o[1] = 0.0; o[2] = 0.0; o[3] = v; o[4] = 0.0; o[5] = v;
    }
    wmask[i] |= (uint8_t)(1u << imet);
  }
}
void launch_const_metric(const int8_t *kind, int64_t nq, double *out, int S, int off, int size,
                         double hsiz, uint8_t *wmask, int imet, hipStream_t s) {
  if (nq < 1) return;
  hipLaunchKernelGGL(k_const_metric, dim3(pmx_grid(nq, 8192)), dim3(256), 0, s, kind, nq, out, S, off,
                     size, hsiz, wmask, imet);
}

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

// One step: one iteration's device work on the uploaded raw arrays -- the
// per-background derived data (with PMX_RUN_FRESH_BACKGROUND, or after an
// upload), the points' classification and compaction, the node -> trias CSR
// (surface points only), hint grids, walks, fallback.  FRESH also redoes
// every device pass of the uploads (rederive: records, samples, face
// matching; the fan check; the orphan marks of the new tets): the step is
// then what a ParMmg iteration costs the device.  pmx_run calls the phases
// in the order they are declared; each enqueues on st (the context's stream),
// side (the surface path), ctx->up (the orphan marks) in the order written.
namespace {
struct Step : pmx_call {
  pmx_run_opts opts{};
  SolDesc sd{};
  int64_t n = 0;                        // the points
  int S = 0;                            // doubles per result row
  bool pm = false;                      // point-map starts (the reference's USE_POINTMAP)
  bool fresh = false, derive = false, csr = false;
  bool marks = false;                   // the orphan marks inside the step (FRESH with new tets)
  bool bdy = false, serial = false;     // surface points; their path on st instead of side
  bool any_interp = false;              // something to interpolate: the points are located
  bool hint_first = false;              // the hint build ahead of the classification, beside the marks
  hipStream_t st, side, ss;             // ss: the surface path's stream (st when serial)
  DevEvent *ev = nullptr;               // the timing events of a timed step
  VolArgs A{};

  Step(pmx_ctx *c, const pmx_run_opts *o) : pmx_call{c, nullptr, c->stream}, st(c->stream), side(c->side), ss(c->side) {
    if (o) opts = *o;
  }
  bool begin();                         // option checks and growth
  bool prefix();                        // prologue, fans, marks, derived data, rederive, point maps
  bool classify_and_hint();             // hint build (when first), classification, constant-size metric
  bool locate();                        // surface fork, hint build, walk, join, fallback, sequential replay
  bool finish();                        // bookkeeping, eager copies, the pending new tets
  void hint_build();
};

bool Step::begin() {
  ctx->ran = false;
  ctx->vgrid_built = ctx->tgrid_built = false;
  ctx->eager_nch = 0;
  if (!ctx->have_bg || !ctx->have_pts) return fail("pmx_run: upload background and points first");
  hipSetDevice(ctx->device);
  if (opts.hint_stride < 0 || opts.max_walk < 0) return fail("pmx_run: bad options");
  if (!run_flags_valid(opts.flags, &ctx->err)) return false;
  // point-map starts: every walk from its point's source vertex.  The
  // sequential modes' speculate-and-replay is built on carried starts:
  // refused together
  pm = (opts.flags & PMX_RUN_POINTMAP) != 0;
  if (pm && (opts.flags & (PMX_RUN_SEQUENTIAL_SURFACE | PMX_RUN_SEQUENTIAL_VOLUME)))
    return fail("pmx_run: PMX_RUN_POINTMAP cannot be combined with PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME");
  if (pm && !ctx->have_src)
    return fail("pmx_run: PMX_RUN_POINTMAP needs the sources of the current points (pmx_upload_point_sources)");
  n = ctx->nq;
  if (pm && (!pmx_dgrow(ctx, ctx->d_pstart, (size_t)std::max<int64_t>(2 * n, 1)) ||
             !pmx_dgrow(ctx, ctx->d_pmap, (size_t)(2 * (ctx->np + 1))) || !pmx_dgrow(ctx, ctx->d_pmcnt, 2)))
    return false;
  S = ctx->sd.S;
  if (!pmx_dgrow(ctx, ctx->d_out, (size_t)std::max<int64_t>(n * S, 1))) return false;
  sd = ctx->sd;
  sd.metric_const = (opts.hsiz > 0.0 && sd.imet >= 0) ? 1 : 0;
  for (int s = 0; s < sd.nsol; s++)
    if (!(s == sd.imet && sd.metric_const)) any_interp = true;
  if (opts.timing && !(ev = ctx->next_event_slot())) return false;
  fresh = (opts.flags & PMX_RUN_FRESH_BACKGROUND) != 0;
  derive = !ctx->have_derived || fresh;
  bdy = ctx->nq_bdy_ub > 0;
  csr = bdy && (!ctx->have_csr || fresh);
  serial = (opts.flags & PMX_RUN_SERIAL_SURFACE) != 0;
  // (r03: the surface stream at the highest priority measured the same,
  // C3 2.093 vs 2.095 ms, profiles/r03_c3_sweep_surface_priority.log)
  ss = serial ? st : side;
  // the marks inside the step: the new tets' DMA must have landed (a pending
  // points view is packed now)
  marks = fresh && ctx->ntets.have && n > 0;
  hint_first = marks && any_interp;
  return !marks || ctx->ntets.ensure_tets(st);
}

bool Step::prefix() {
  if (ev) PMX_CK(*this, hipEventRecord(ev[0], st));
  // one prologue kernel zeroes the write masks, the counters and the hint grid
  ZeroRanges z{};
  z.add(ctx->d_wmask.p, n);
  z.add(ctx->d_counts.p, 32 * sizeof(unsigned));
  if (!pm) z.add(ctx->d_grid.p, ctx->gcells * (int64_t)sizeof(int));
  launch_prologue(z, st);
  // the node -> trias fans (PMMG_precompute_nodeTrias, surface points only)
  // on the side stream from the start of the step: a small radix sort that
  // overlaps the derived data, the classification and the hint build
  if (bdy && !serial) {
    PMX_CK(*this, hipEventRecord(ctx->ev_fork, st));
    PMX_CK(*this, hipStreamWaitEvent(side, ctx->ev_fork, 0));
  }
  // (on the side stream only once it has been forked from the main one: an
  // unforked side stream's event could precede ev[0])
  if (ev) PMX_CK(*this, hipEventRecord(ev[3], bdy ? ss : st));
  if (csr) {
    if (!ctx->build_node_trias(ss, fresh)) return false;
    ctx->have_csr = true;
  }
  // the orphan marks on `up`, beside the derived data and the hint build
  // (the classification waits for them)
  if (marks && !ctx->ntets.step_marks(st)) return false;
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
  if (fresh && !ctx->rederive(st)) return false;
  if (ev) PMX_CK(*this, hipEventRecord(ev[7], st));
  // the first-incident-element maps: derived background data like the tria
  // normals, after the records a FRESH step rebuilt, only for a flagged step
  if (ev) PMX_CK(*this, hipEventRecord(ev[8], st));
  if (pm && (!ctx->have_pmap || fresh)) {
    launch_pmap_build(ctx->d_tets.p, ctx->ne, ctx->d_tris.p, ctx->nt, ctx->np, ctx->d_pmap.p, ctx->d_pmcnt.p, st);
    ctx->have_pmap = true;
  }
  if (ev) PMX_CK(*this, hipEventRecord(ev[9], st));
  return true;
}

// the volume hint grid on st (point-map starts: no grid, the starts come with
// the classification)
void Step::hint_build() {
  if (pm) return;
  const int stride = opts.hint_stride > 0 ? opts.hint_stride : PMX_HINT_STRIDE;
  const bool packed = stride == PMX_HINT_STRIDE;
  launch_hint_build(packed ? ctx->d_tets_s.p : nullptr,
                    packed && ctx->samples_sorted ? ctx->d_tets_sk.p : nullptr, ctx->d_tets.p, ctx->ne,
                    stride, ctx->d_grid.p, ctx->grid, ctx->d_xyzq.p, st,
                    packed && ctx->samples_owner ? ctx->nsamp : -1);
  ctx->vgrid_built = true;
}

bool Step::classify_and_hint() {
  // with the marks in the step, the hint build (which does not depend on the
  // points) goes ahead of the classification, beside the marks
  if (hint_first) hint_build();
  if (marks) PMX_CK(*this, hipStreamWaitEvent(st, ctx->ntets.ev, 0));
  if (!ctx->classify(st, marks, pm)) return false;
  if (sd.metric_const)
    launch_const_metric(ctx->d_kind.p, n, ctx->d_out.p, S, sd.off[sd.imet], sd.size[sd.imet],
                        opts.hsiz, ctx->d_wmask.p, sd.imet, st);
  return true;
}

bool Step::locate() {
  if (!any_interp) {
    // reference early exit (src/interpmesh_pmmg.c:508-512): nothing to locate
    if (bdy && !serial) {
      PMX_CK(*this, hipEventRecord(ctx->ev_join, side));
      PMX_CK(*this, hipStreamWaitEvent(st, ctx->ev_join, 0));
    }
    if (ev)
      for (int k = 1; k < PMX_EV_PER_RUN; k++)
        if (k != 7 && k != 3 && k != 8 && k != 9) PMX_CK(*this, hipEventRecord(ev[k], st));
    PMX_CK(*this, hipGetLastError());
    return true;
  }
  fill_vol_args(ctx, sd, opts, A);
  // the surface path on the side stream as soon as the points are
  // classified, latency-bound beside the hint build and the volume walk
  // (r03 A/B, profiles/r03_c{2,3,4}_sweep_surface_fork.log: C2 step 0.346 ->
  // 0.338 ms, C3 / C4 within 0.1 %)
  if (bdy && !serial) {
    PMX_CK(*this, hipEventRecord(ctx->ev_fork2, st));
    PMX_CK(*this, hipStreamWaitEvent(side, ctx->ev_fork2, 0));
    if (!ctx->launch_bdy(A, side, pm)) return false;
    if (ev) PMX_CK(*this, hipEventRecord(ev[5], side));
    PMX_CK(*this, hipEventRecord(ctx->ev_join, side));
  }
  if (!hint_first) hint_build();
  if (ev) PMX_CK(*this, hipEventRecord(ev[1], st));
  if (ctx->nq_vol_ub) launch_walk(A, st, pm);
  if (ev) PMX_CK(*this, hipEventRecord(ev[2], st));
  if (bdy && !serial) {
    PMX_CK(*this, hipStreamWaitEvent(st, ctx->ev_join, 0));     // surface path done
  } else if (bdy) {
    if (!ctx->launch_bdy(A, st, pm)) return false;
    if (ev) PMX_CK(*this, hipEventRecord(ev[5], st));
  } else if (ev) {
    PMX_CK(*this, hipEventRecord(ev[5], st));
  }
  if (ev) PMX_CK(*this, hipEventRecord(ev[6], st));
  ExhArgs E{};
  E.xyz = ctx->d_xyz.p; E.tets = ctx->d_tets.p; E.ne = ctx->ne; E.q = ctx->d_qxyz.p;
  E.list = ctx->d_list.p; E.count = ctx->d_counts.p; E.found = ctx->d_found.p;
  E.best = ctx->d_best.p; E.bestk = ctx->d_bestk.p;
  E.spin_limit = (opts.flags & PMX_RUN_DEBUG_BARRIER_TIMEOUT) ? 0L : (1L << 26);
  const int share = std::max(2, live_contexts(ctx->device).load());
  if (share != ctx->fallback_share) {
    const int fb = fallback_coresident_blocks(ctx->device, share);
    if (fb < 1) return fail("pmx_run: occupancy query failed");
    ctx->fallback_blocks = fb;
    ctx->fallback_share = share;
  }
  if (ctx->nq_vol_ub) launch_exhaustive(E, A, ctx->fallback_blocks, st);
  // the reference's sequential semantics, after every default result
  ctx->seq_stats_n = -1;   // "seq_stats_n is reset to -1 only inside the branch that runs the walks" (kept as it is)
  const bool sq_s = bdy && (opts.flags & PMX_RUN_SEQUENTIAL_SURFACE);
  const bool sq_v = ctx->nq_vol_ub > 0 && (opts.flags & PMX_RUN_SEQUENTIAL_VOLUME);
  if (opts.flags & (PMX_RUN_SEQUENTIAL_SURFACE | PMX_RUN_SEQUENTIAL_VOLUME)) {
    if (!ctx->seq_replay(A, st, sq_s, sq_v)) return false;
    ctx->seq_stats_n = 1;
  }
  if (ev) PMX_CK(*this, hipEventRecord(ev[4], st));
  PMX_CK(*this, hipGetLastError());
  return true;
}

// The new tets of the points view are packed and sent now, while the device
// runs the step.
bool Step::finish() {
  ctx->ntets.step_done(marks, sd.metric_const ? (1u << sd.imet) : 0u);
  ctx->out_S = S;
  ctx->out_n = n;
  ctx->located = any_interp;
  if ((opts.flags & PMX_RUN_EAGER_DOWNLOAD) && !ctx->eager_download()) return false;
  if (!ctx->ntets.pack_new_tets()) return false;
  ctx->ran = true;
  return true;
}

}  // namespace

extern "C" int pmx_run(pmx_ctx *ctx, const pmx_run_opts *o) {
  if (!ctx) return 0;
  Step s(ctx, o);
  return s.begin() && s.prefix() && s.classify_and_hint() && s.locate() && s.finish();
}

// The fields and write masks of the step just enqueued, down into h_out (its
// own pinned buffer: the arena stays free for the calls in between) in chunks
// on the step's stream.  The orphan reset (fix_orphans, later) changes masks
// only: pmx_download takes them again.
bool pmx_ctx::eager_download() {
  const pmx_call C{this};
  eager_nch = 0;
  const int64_t n = nq;
  const int S = sd.S;
  if (n == 0 || S == 0) return true;
  const size_t o_wm = pmx_call::al256((size_t)(n * S) * sizeof(double)), bytes = o_wm + pmx_call::al256((size_t)n);
  if (bytes > h_out.cap) {
    PMX_CK(C, hipStreamSynchronize(stream));      // an earlier eager copy may still land in it
    if (!C.ok(h_out.grow(bytes, bytes + bytes / 4), "pmx_run: pinned staging of the eager download")) return false;
  }
  const int nch = (int)std::max<int64_t>(1, std::min<int64_t>(4, (n * S) >> 21));
  for (int c = 0; c < nch; c++) {
    const int64_t lo = n * c / nch, hi = n * (c + 1) / nch;
    PMX_CK(C, hipMemcpyAsync(h_out.p + (size_t)(lo * S) * sizeof(double), d_out.p + lo * S,
                             (size_t)((hi - lo) * S) * sizeof(double), hipMemcpyDeviceToHost, stream));
    PMX_CK(C, hipMemcpyAsync(h_out.p + o_wm + lo, d_wmask.p + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, stream));
    PMX_CK(C, hipEventRecord(ev_eg[c], stream));
  }
  eager_nch = nch;
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

extern "C" {

int pmx_timing_reset(pmx_ctx *ctx) {
  if (!ctx) return 0;
  ctx->ev_used = 0;
  return 1;
}

double pmx_kernel_ms(pmx_ctx *ctx, int which) {
  if (ctx && which == 7) return pmx_more_kernel_ms(ctx);
  if (ctx && which >= 8 && which <= 11) return pmx_graph_kernel_ms(ctx, which);
  if (ctx && (which == 12 || which == 13)) return pmx_contig_kernel_ms(ctx, which);
  if (ctx && (which == 14 || which == 15 || which == 21)) return pmx_split_kernel_ms(ctx, which);
  if (ctx && which >= 16 && which <= 18) return pmx_merge_kernel_ms(ctx, which);
  if (ctx && (which == 19 || which == 20)) return pmx_moveifc_kernel_ms(ctx, which);
  if (ctx && (which == 22 || which == 23)) return pmx_reach_kernel_ms(ctx, which);
  if (ctx && which == 24) return pmx_part_kernel_ms(ctx);
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

}  // extern "C"
