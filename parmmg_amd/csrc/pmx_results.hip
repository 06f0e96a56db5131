// pmx_results.hip -- the last step's results on the host: the downloads
// (fields, elements, starts, border entities, the new mesh's qualities) and
// the statistics getters.  Every results call starts with results_begin.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "pmx_transfer.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"

// The preamble of a results call: a step has run on the current uploads, the
// caller's arrays hold `need` entries (refused before anything is written --
// r04: an output sized by a wrong count was written past on the host), the
// orphans' rows are reset, the stream has drained and the step's device error
// word is clear.  A call without a host array passes cap = need = 0.
static bool results_begin(pmx_ctx *ctx, const char *who, int64_t cap, int64_t need) {
  const pmx_call C{ctx, who, ctx->stream};
  if (!ctx->stepped() || !ctx->have_bg || ctx->out_S != ctx->sd.S)
    return C.fail("no step has run on the current uploads");
  if (cap < need)
    return C.fail("output capacity " + std::to_string(cap) + " < " + std::to_string(need) + " entries needed");
  (void)hipSetDevice(ctx->device);
  if (!ctx->ntets.fix_orphans()) return false;
  PMX_CK(pmx_call{ctx}, hipStreamSynchronize(ctx->stream));
  return ctx->check_device_errors();
}

// [0, n) in nch chunks: where chunk c begins
static inline int64_t chunk_at(int64_t n, int64_t c, int64_t nch) { return n * c / nch; }
// chunks sent down with an event each: f(lo, hi) on each one once it has
// landed, while the DMA of the next goes on
template <class F> static bool consume_chunks(pmx_ctx *ctx, const DevEvent *ev, int64_t n, int64_t nch, F f) {
  for (int64_t c = 0; c < nch; c++) {
    PMX_CK(pmx_call{ctx}, hipEventSynchronize(ev[c]));
    f(chunk_at(n, c, nch), chunk_at(n, c + 1, nch));
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

bool pmx_download_qual(pmx_ctx *ctx, const double *dev, int64_t ne, double *qual, int64_t stride) {
  const pmx_call C{ctx};
  const bool dense = stride == (int64_t)sizeof(double);
  const int4 *htv = (const int4 *)ctx->ntets.h.p;
  if (!dense && (!htv || ctx->ntets.h.cap < (size_t)(ne + 1) * sizeof(int4)))
    return C.fail("qualities: strided output needs the new tets' host copy");
  hipStream_t s = ctx->stream;
  char *st = pmx_hstage(ctx, (size_t)(ne + 1) * sizeof(double));
  if (!st) return false;
  const double *h = (const double *)st;
  char *out = (char *)qual;
  const bool nt_q = !dense && ((uintptr_t)out % 8) == 0 && stride % 8 == 0;
  const int64_t nch = std::max<int64_t>(1, std::min<int64_t>(8, (ne + 1) >> 20));
  for (int64_t c = 0; c < nch; c++) {
    const int64_t lo = chunk_at(ne + 1, c, nch), hi = chunk_at(ne + 1, c + 1, nch);
    PMX_CK(C, hipMemcpyAsync(st + lo * 8, dev + lo, (size_t)(hi - lo) * 8, hipMemcpyDeviceToHost, s));
    PMX_CK(C, hipEventRecord(ctx->ev_dl[c], s));
  }
  const bool ok = consume_chunks(ctx, ctx->ev_dl, ne + 1, nch, [&](int64_t lo, int64_t hi) {
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
  });
  if (!ok) return false;
  if (dense) qual[0] = 0.0;
  return true;
}

extern "C" {

// Every device -> host copy lands in pinned memory (async DMA), then the host
// scatters into the caller's (pageable, strided) arrays.  The fields and
// write masks come down in chunks with an event each, a chunk's scatter
// overlapping the DMA of the next: into the arena, issued here -- or, after a
// PMX_RUN_EAGER_DOWNLOAD step, into h_out, issued by that step (eager_download).
int pmx_download(pmx_ctx *ctx, const pmx_sol_view *new_sols, int64_t npts_cap, int *elem, int *status,
                 int *steps) {
  if (!ctx) return 0;
  if (!results_begin(ctx, "pmx_download", npts_cap, ctx->nq)) return 0;
  const pmx_call C{ctx};
  const int64_t n = ctx->nq;
  const int S = ctx->sd.S;
  if (n == 0) return 1;   // empty step: nothing to copy
  hipStream_t s = ctx->stream;
  const bool want_sol = new_sols && S > 0;
  const bool eager = want_sol && ctx->eager_nch > 0;
  const bool arena_sol = want_sol && !eager;
  int *const dst[3] = {elem, status, steps};
  const int *const src[3] = {ctx->d_elem.p, ctx->d_status.p, ctx->d_steps.p};
  const size_t fbytes = pmx_call::al256((size_t)(n * S) * sizeof(double)), ibytes = pmx_call::al256((size_t)n * sizeof(int));
  // the arena: fields | masks (unless they are in h_out) | elem | status | steps
  const size_t o_wm = arena_sol ? fbytes : 0, o_int = o_wm + pmx_call::al256(arena_sol ? (size_t)n : 0);
  const char *fields = nullptr;
  const DevEvent *ev = ctx->ev_dl;
  int64_t nch = 0;
  if (eager) {
    fields = ctx->h_out.p;
    ev = ctx->ev_eg;
    nch = ctx->eager_nch;
    // the eager copy holds the step's masks; with new tets, the orphan reset
    // (fix_orphans, enqueued above, after them) changed some: take the masks
    // again (n bytes)
    if (ctx->ntets.marks) {
      PMX_CK(C, hipMemcpyAsync(ctx->h_out.p + fbytes, ctx->d_wmask.p, (size_t)n, hipMemcpyDeviceToHost, s));
      PMX_CK(C, hipStreamSynchronize(s));
    }
  }
  // the eager path takes the arena (which drains the stream: its chunks have
  // landed) only when an int array is asked for
  char *st = nullptr;
  if (!eager || elem || status || steps) {
    st = pmx_hstage(ctx, o_int + 3 * ibytes);
    if (!st) return 0;
  }
  if (arena_sol) {
    fields = st;
    nch = std::max<int64_t>(1, std::min<int64_t>(4, (n * S) >> 21));
    for (int64_t c = 0; c < nch; c++) {
      const int64_t lo = chunk_at(n, c, nch), hi = chunk_at(n, c + 1, nch);
      PMX_CK(C, hipMemcpyAsync(st + (size_t)(lo * S) * sizeof(double), ctx->d_out.p + lo * S,
                               (size_t)((hi - lo) * S) * sizeof(double), hipMemcpyDeviceToHost, s));
      PMX_CK(C, hipMemcpyAsync(st + o_wm + lo, ctx->d_wmask.p + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, s));
      PMX_CK(C, hipEventRecord(ev[c], s));
    }
  }
  for (int k = 0; k < 3; k++)
    if (dst[k]) PMX_CK(C, hipMemcpyAsync(st + o_int + k * ibytes, src[k], (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
  const double *h = (const double *)fields;
  const uint8_t *wm = fields ? (const uint8_t *)(fields + fbytes) : nullptr;
  if (!consume_chunks(ctx, ev, n, nch, [&](int64_t lo, int64_t hi) {
        par_for(lo, hi, [&](int64_t i0, int64_t i1) { scatter_rows(ctx, new_sols, h, wm, i0, i1); });
      }))
    return 0;
  if (st) PMX_CK(C, hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++)
    if (dst[k]) memcpy(dst[k], st + o_int + k * ibytes, (size_t)n * sizeof(int));
  return 1;
}

int pmx_download_starts(pmx_ctx *ctx, int *start, int64_t cap) {
  if (!ctx || !start) return 0;
  if (!results_begin(ctx, "pmx_download_starts", cap, ctx->nq)) return 0;
  if (ctx->nq == 0) return 1;
  PMX_CK(pmx_call{ctx}, hipMemcpy(start, ctx->d_start.p, (size_t)ctx->nq * sizeof(int), hipMemcpyDeviceToHost));
  return 1;
}

int pmx_download_border(pmx_ctx *ctx, int *edge, int *vertex, int64_t cap) {
  if (!ctx) return 0;
  if (!results_begin(ctx, "pmx_download_border", cap, ctx->nq)) return 0;
  const pmx_call C{ctx};
  if (ctx->nq == 0) return 1;
  if (edge) PMX_CK(C, hipMemcpy(edge, ctx->d_edge.p, (size_t)ctx->nq * sizeof(int), hipMemcpyDeviceToHost));
  if (vertex) PMX_CK(C, hipMemcpy(vertex, ctx->d_vertex.p, (size_t)ctx->nq * sizeof(int), hipMemcpyDeviceToHost));
  return 1;
}

int pmx_locate_stats_get(pmx_ctx *ctx, pmx_locate_stats *st) {
  if (!ctx || !st) return 0;
  if (!results_begin(ctx, "pmx_locate_stats_get", 0, 0)) return 0;
  const pmx_call C{ctx};
  // per point, over the points the reference visits (kind VOL / BDY; orphans
  // are KIND_ORPH once fix_orphans has run, NUL / frozen points never
  // located): steps > 0 located by a walk, steps < 0 by an exhaustive scan
  // (the reference's ppt->s sign, src/locate_pmmg.c:840-844), status 0 the
  // closest element (not contained anywhere)
  const int64_t n = ctx->nq;
  std::vector<int> status((size_t)std::max<int64_t>(n, 1)), steps((size_t)std::max<int64_t>(n, 1));
  std::vector<int8_t> kind((size_t)std::max<int64_t>(n, 1));
  if (n) {
    PMX_CK(C, hipMemcpy(status.data(), ctx->d_status.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PMX_CK(C, hipMemcpy(steps.data(), ctx->d_steps.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    PMX_CK(C, hipMemcpy(kind.data(), ctx->d_kind.p, (size_t)n, hipMemcpyDeviceToHost));
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
  if (!results_begin(ctx, "pmx_locate_wave_stats", 0, 0)) return 0;
  const pmx_call C{ctx};
  int nsel[2] = {0, 0};
  if (ctx->nq) PMX_CK(C, hipMemcpy(nsel, ctx->d_nsel.p, sizeof nsel, hipMemcpyDeviceToHost));
  memset(st, 0, sizeof *st);
  const int64_t npath = nsel[path];
  if (!npath) return 1;
  std::vector<uint4> w((size_t)((npath + 255) / 256 * 4));
  PMX_CK(C, hipMemcpy(w.data(), path ? ctx->d_bstat.p : ctx->d_vstat.p, w.size() * sizeof(uint4),
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

// surface replays / sequence (which = 0), volume replays / sequence (which = 2)
static int seq_stats_get(pmx_ctx *ctx, const char *who, int which, int64_t *nseq, int64_t *nreplay) {
  if (!ctx || !nseq || !nreplay) return 0;
  if (ctx->seq_stats_n < 0 || !ctx->ran)
    return pmx_call{ctx, who}.fail("the last step did not run PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME");
  *nseq = ctx->seq_stats[which + 1];
  *nreplay = ctx->seq_stats[which];
  return 1;
}
int pmx_seq_surface_stats(pmx_ctx *ctx, int64_t *nseq, int64_t *nreplay) {
  return seq_stats_get(ctx, "pmx_seq_surface_stats", 0, nseq, nreplay);
}
int pmx_seq_volume_stats(pmx_ctx *ctx, int64_t *nseq, int64_t *nreplay) {
  return seq_stats_get(ctx, "pmx_seq_volume_stats", 2, nseq, nreplay);
}

int pmx_step_ready(pmx_ctx *ctx) {
  return ctx && ctx->stepped() && ctx->have_bg && ctx->out_S == ctx->sd.S;
}

void *pmx_device_buffer(pmx_ctx *ctx, int which) {
  if (!ctx) return nullptr;
  // the orphan rows reset before a caller chains on the results (enqueued on
  // the context stream, which the caller orders its own work after)
  if (ctx->ran && (which == 0 || which == 1 || which == 2)) {
    (void)hipSetDevice(ctx->device);
    if (!ctx->ntets.fix_orphans()) return nullptr;
  }
  switch (which) {
    case 0: return ctx->d_out.p;
    case 1: return ctx->d_elem.p;
    case 2: return ctx->d_status.p;
    default: return nullptr;
  }
}

int64_t pmx_debug_hint_grid(pmx_ctx *ctx, int *host, int64_t cap) {
  if (!ctx || !ctx->ran || !host) return 0;
  const pmx_call C{ctx};
  PMX_CK(C, hipStreamSynchronize(ctx->stream));
  const int64_t n = std::min<int64_t>(cap, ctx->gcells);
  PMX_CK(C, hipMemcpy(host, ctx->d_grid.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
  return ctx->gcells;
}

int64_t pmx_debug_grid(pmx_ctx *ctx, int which, pmx_grid_desc *desc, int *cells, int64_t cap) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_debug_grid", ctx->stream};
  if (which != 0 && which != 1) return C.fail("which is 0 (volume grid) or 1 (tria grid)"), 0;
  if (!ctx->ran || !ctx->have_bg) return C.fail("no step has run on the current background"), 0;
  if (!(which ? ctx->tgrid_built : ctx->vgrid_built))
    return C.fail(which ? "the last step built no tria hint grid" : "the last step built no volume hint grid"), 0;
  const GridDesc &g = which ? ctx->tgd : ctx->grid;
  const int64_t n = which ? ctx->tcells : ctx->gcells;
  if (desc)
    for (int a = 0; a < 3; a++) {
      desc->dim[a] = g.dim[a];
      desc->qf[a] = which ? 0 : g.qf[a];     // the tria grid has no fixed-point coordinates
      desc->lo[a] = g.lo[a];
      desc->inv[a] = g.inv[a];
    }
  if (!cells) return n;                      // the size query
  if (cap < n) return C.fail("more cells than cap"), 0;
  (void)hipSetDevice(ctx->device);
  if (!C.sync("stream") ||
      !C.hip(hipMemcpy(cells, which ? ctx->d_tgrid.p : ctx->d_grid.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost),
             "download"))
    return 0;
  return n;
}

int pmx_pointmap_stats(pmx_ctx *ctx, int64_t atomics[2]) {
  if (!ctx || !atomics) return 0;
  const pmx_call C{ctx};
  if (!ctx->have_pmap) return C.fail("pmx_pointmap_stats: no PMX_RUN_POINTMAP step on this background");
  (void)hipSetDevice(ctx->device);
  PMX_CK(C, hipStreamSynchronize(ctx->stream));
  unsigned c[2] = {0, 0};
  PMX_CK(C, hipMemcpy(c, ctx->d_pmcnt.p, sizeof c, hipMemcpyDeviceToHost));
  atomics[0] = c[0];
  atomics[1] = c[1];
  return 1;
}

}  // extern "C"
