// pmx_points.hip -- the new points and the new tets (host side).
//
// pmx_upload_points / pmx_upload_point_sources, the points' classification,
// and NewTets: the new mesh's tets on the device with the orphan reset that
// depends on them.  Every assignment to a NewTets member is in this file; its
// states and transitions are the table at the struct (pmx_internal.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>

#include "pmx_transfer.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"

// ---- the new tets ---------------------------------------------------------------

// One row of the caller's new tets (vertices are view indices first ..
// first + n - 1) as the packed record, vertex = view index - first + 1; a
// deleted row (v[0] <= 0, !MG_EOK) is all zero.  A vertex outside the view
// sets *bad and packs as vertex 1 (the call then fails).
static inline int4 pack_tet_row(const int *v, int64_t first, int64_t n, bool *bad) {
  if (v[0] <= 0) return make_int4(0, 0, 0, 0);
  int w[4];
  for (int l = 0; l < 4; l++) {
    int64_t j = (int64_t)v[l] - first;
    if (j < 0 || j >= n) { *bad = true; j = 0; }
    w[l] = (int)(j + 1);
  }
  return make_int4(w[0], w[1], w[2], w[3]);
}

// rows [k0, k1) of tc into the pinned records h (streaming stores, fenced);
// true when a vertex was outside the view
static bool pack_tet_rows(const char *tc, int64_t stride, int64_t first, int64_t n, int4 *h, int64_t k0, int64_t k1) {
  bool bad = false;
  par_for(k0, k1, [&](int64_t a, int64_t b) {
    bool bd = false;
    for (int64_t k = a; k < b; k++) {
      const int4 r = pack_tet_row((const int *)(tc + k * stride), first, n, &bd);
      st4(&h[k], r.x, r.y, r.z, r.w);
    }
    if (bd) __atomic_store_n(&bad, true, __ATOMIC_RELAXED);
    std::atomic_thread_fence(std::memory_order_seq_cst);
  });
  return bad;
}

bool NewTets::drain() {
  if (!inflight) return true;
  PMX_CK(pmx_call{ctx}, hipEventSynchronize(ev));
  inflight = false;
  return true;
}

bool NewTets::drop_next() {
  if (!next_topo) return true;
  PMX_CK(pmx_call{ctx}, hipStreamSynchronize(ctx->topo));
  next_topo = false;
  return true;
}

// the tets belong to the points: none from here on; d_v, h and the residency
// build's buffers are about to be reused
bool NewTets::points_begin() {
  have = false;
  if (!drop_next() || !drain()) return false;
  pending = false;
  marks = false;
  rows_reset = true;
  return true;
}

// the view's tets are packed and sent by the first step on these points
// (pack_new_tets): their DMA overlaps the step and the download
void NewTets::view_kept(const pmx_points_view &pv, int64_t ntet) {
  view = pv;
  pending = from_view = have = ntet > 0;
  n = ntet;
}

bool NewTets::take_next(bool wanted) {
  const bool prepared = next_topo && wanted;
  next_topo = false;
  return prepared;
}

void NewTets::consumed() { have = false; }

int4 *NewTets::grow_htets(int64_t ne) {
  const size_t bytes = (size_t)(ne + 1) * sizeof(int4);
  if (!pmx_call{ctx}.ok(h.grow(bytes, bytes), "pinned staging of the new tets")) return nullptr;
  return (int4 *)h.p;
}

bool NewTets::mark_new_tets(int64_t ne, hipStream_t s) {
  const pmx_call C{ctx};
  if (ctx->nq < 1) return true;
  PMX_CK(C, hipMemsetAsync(d_mark.p, 0, (size_t)ctx->nq, s));
  launch_mark_new_tets(d_v.p, ne, d_mark.p, ctx->nq, s);
  PMX_CK(C, hipGetLastError());
  return true;
}

// The points view's new tets, validated and packed in chunks into their own
// pinned staging (the shared arena serves the download meanwhile), each
// chunk's DMA on `up` overlapping the packing of the next.  Once they are on
// the device, a kernel on the same stream marks the points of valid tets, so
// that the points in no valid tet (orphans: untouched, the reference never
// visits them) are known to fix_orphans.  With residency the next
// background's tet records are built from them on the topo stream once they
// have arrived.
bool NewTets::pack_new_tets() {
  const pmx_call C{ctx};
  if (!pending) return true;
  pending = false;
  const pmx_points_view *pv = &view;
  const int64_t nq = ctx->nq, ntet = pv->ne;
  hipStream_t up = ctx->up, topo = ctx->topo;
  Trace tr("new tets");
  int4 *htv = grow_htets(ntet);
  if (!htv) return false;
  const char *tc = (const char *)pv->tetra_v;
  bool bad = false;
  htv[0] = make_int4(0, 0, 0, 0);
  const int64_t nch = std::max<int64_t>(1, std::min<int64_t>(8, ntet >> 20));
  for (int64_t c = 0; c < nch && !bad; c++) {
    const int64_t lo = (c == 0) ? 0 : 1 + ntet * c / nch, hi = 1 + ntet * (c + 1) / nch;
    bad = pack_tet_rows(tc, pv->tetra_stride, pv->first, nq, htv, std::max<int64_t>(lo, 1), hi);
    if (!bad)
      PMX_CK(C, hipMemcpyAsync(d_v.p + lo, htv + lo, (size_t)(hi - lo) * sizeof(int4), hipMemcpyHostToDevice, up));
  }
  if (!bad && nq > 0) {
    // the orphan marks, on the device once the tets are there (the host's
    // byte stores into a point-sized array cost as much as the packing)
    if (!mark_new_tets(ntet, up)) return false;
    marks = true;
  }
  PMX_CK(C, hipEventRecord(ev, up));
  inflight = true;
  if (bad) {
    have = false;
    return C.fail("pmx_run: new tet vertex outside [first, last] of the points view");
  }
  tr.mark("pack + dma issued");
  // residency: the next background's tet records (face adjacency built on
  // the device) on the topo stream, after the tets' DMA, while the step and
  // the download go on
  if (ctx->residency && ntet > 0) {
    PMX_CK(C, hipStreamWaitEvent(topo, ev, 0));
    if (!ctx->build_records(d_v.p, nullptr, ntet, nq, ctx->records_next(), topo)) return false;
    PMX_CK(C, hipEventRecord(ev_topo, topo));
    next_topo = true;
  }
  return true;
}

bool NewTets::ensure_tets(hipStream_t s) {
  if (pending && !pack_new_tets()) return false;
  if (inflight) PMX_CK(pmx_call{ctx}, hipStreamWaitEvent(s, ev, 0));
  return true;
}

// the orphan marks inside a FRESH step, on `up` beside the derived data and
// the hint build (the classification waits for ev)
bool NewTets::step_marks(hipStream_t st) {
  const pmx_call C{ctx};
  PMX_CK(C, hipEventRecord(ctx->ev_fork, st));
  PMX_CK(C, hipStreamWaitEvent(ctx->up, ctx->ev_fork, 0));
  if (!mark_new_tets(n, ctx->up)) return false;
  PMX_CK(C, hipEventRecord(ev, ctx->up));
  inflight = true;
  return true;
}

// The step located every live point: the orphans' rows are reset by the first
// consumer of its results (fix_orphans).  With the marks in the step the
// orphans were never located (KIND_ORPH): nothing to reset.
void NewTets::step_done(bool marks_in_step, unsigned step_const_bit) {
  const_bit = step_const_bit;
  rows_reset = marks_in_step;   // "orph_fixed = marks" after a FRESH step (kept as it is)
  if (marks_in_step) marks = true;
}

// The orphans' rows go back to "never visited" -- no written solution bit (a
// constant-size metric stays: MMG3D_Set_constantSize writes every valid
// point), element / status / steps 0 -- on the stream, before any consumer of
// the results.
bool NewTets::fix_orphans() {
  const pmx_call C{ctx};
  if (rows_reset) return true;
  rows_reset = true;
  if (!ctx->ran || !marks || ctx->nq == 0) return true;
  if (inflight) PMX_CK(C, hipStreamWaitEvent(ctx->stream, ev, 0));   // the marks are written on `up`
  OrphanRows r{ctx->d_wmask.p, ctx->d_elem.p, ctx->d_status.p, ctx->d_steps.p,
               ctx->d_start.p, ctx->d_edge.p,  ctx->d_vertex.p, ctx->d_kind.p};
  launch_orphans(d_mark.p, ctx->nq, (uint8_t)const_bit, r, ctx->stream);
  PMX_CK(C, hipGetLastError());
  return true;
}

// pmx_upload_new_tets: these tets replace the points view's (if any)
bool NewTets::replace(const int *tetra_v, int64_t tetra_stride, int64_t ne) {
  const pmx_call C{ctx};
  const int64_t first = ctx->pts_first, nq = ctx->nq;
  const char *tc = (const char *)tetra_v;
  if (ctx->ran && from_view) {
    // the last step took its orphans from the points view's tets (never
    // located, or located and reset): other tets would need another step.
    // The same tets are accepted (their pinned copy, packed by that step, is
    // compared row by row); nothing changes on a refusal.
    if (!drain()) return false;
    const int4 *old = (const int4 *)h.p;
    bool same = old && !pending && ne == view.ne;
    for (int64_t k = 1; same && k <= ne; k++) {
      bool bad = false;
      const int4 r = pack_tet_row((const int *)(tc + k * tetra_stride), first, nq, &bad);
      if (bad) return C.fail("pmx_upload_new_tets: tet vertex outside the uploaded points");
      const int4 o = old[k];
      same = o.x == r.x && o.y == r.y && o.z == r.z && o.w == r.w;
    }
    if (!same)
      return C.fail("pmx_upload_new_tets: the last step took its orphans from the points view's new tets; "
                    "other tets need another pmx_run");
  }
  have = false;
  if (!drop_next()) return false;          // built from other tets: drop it
  pending = false;                         // these tets replace the points view's
  if (!drain()) return false;
  // packed into the pinned copy of the new tets (a strided quality output
  // reads their validity there), vertices renumbered from the points view
  // (first..last) to 1..n: the numbering of a promoted background
  int4 *hv = grow_htets(ne);
  if (!hv) return false;
  hv[0] = make_int4(0, 0, 0, 0);
  if (pack_tet_rows(tc, tetra_stride, first, nq, hv, 1, ne + 1))
    return C.fail("pmx_upload_new_tets: tet vertex outside the uploaded points");
  if (!pmx_dgrow(ctx, d_v, (size_t)(ne + 1))) return false;
  PMX_CK(C, hipMemcpyAsync(d_v.p, hv, (size_t)(ne + 1) * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
  if (from_view && nq > 0) {
    // the reference visits the points of THESE tets' valid ones
    // (src/interpmesh_pmmg.c:535-541), so the orphan marks come from them (a
    // step already run has its orphan rows reset from these marks by the next
    // consumer of its results)
    if (!mark_new_tets(ne, ctx->stream)) return false;
    marks = true;
    if (ctx->ran) rows_reset = false;
  }
  PMX_CK(C, hipStreamSynchronize(ctx->stream));
  n = ne;
  have = true;
  return true;
}

// ---- the new points ---------------------------------------------------------------

extern "C" {

int pmx_upload_points(pmx_ctx *ctx, const pmx_points_view *pv) {
  if (!ctx) return 0;
  const pmx_call C{ctx};
  ctx->have_pts = ctx->ran = false;
  ctx->have_src = false;                   // the source vertices belong to the points, as the new tets do
  Trace tr("points");
  if (!ctx->ntets.points_begin()) return 0;
  ctx->eager_nch = 0;
  if (!pv) return C.fail("pmx_upload_points: null view");
  (void)hipSetDevice(ctx->device);
  const int64_t n = pv->last - pv->first + 1;
  if (n < 0 || n >= (1LL << 31) || pv->first < 0 || (n > 0 && (!pv->c || pv->stride < 24)))
    return C.fail("pmx_upload_points: bad range or coordinates");
  if (pv->tetra_v && (pv->ne < 0 || pv->tetra_stride < 16)) return C.fail("pmx_upload_points: bad new-tet view");
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
  PMX_CK(C, hipStreamSynchronize(ctx->stream));   // the arena may still feed an earlier copy
  char *st = pmx_hstage(ctx, total);
  if (!st) return 0;
  double *hx = (double *)(st + o_x);
  uint16_t *htg = (uint16_t *)(st + o_tg);
  const char *pc = (const char *)pv->c;
  const char *tg = (const char *)pv->tag;
  if (!pmx_dgrow(ctx, ctx->d_qxyz, nn * 3) || !pmx_dgrow(ctx, ctx->d_kind, nn) ||
      !pmx_dgrow(ctx, ctx->ntets.d_mark, nn + 64) ||   // + 64: the marks' word-wide flush
      !pmx_dgrow(ctx, ctx->d_nsel, 2) || !pmx_dgrow(ctx, ctx->d_vollist, nn) || !pmx_dgrow(ctx, ctx->d_bdylist, nn) ||
      !pmx_dgrow(ctx, ctx->d_ctile, (size_t)std::max<int64_t>(cls_tiles(n), 1)) ||
      (tg && !pmx_dgrow(ctx, ctx->d_qtag, nn)) || (ntet && !pmx_dgrow(ctx, ctx->ntets.d_v, (size_t)(ntet + 1))))
    return 0;
  // coordinates (+ bounding box: a promoted background's hint grid) and tags
  // (+ the per-path upper bounds)
  double qlo[64][3], qhi[64][3];
  int64_t cvol[64], cbdy[64];
  const int nc = par_chunks(0, n, [&](int ci, int64_t j0, int64_t j1) {
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
  for (int i = 0; i < nc; i++) {
    ctx->nq_vol_ub += cvol[i];
    ctx->nq_bdy_ub += cbdy[i];
  }
  for (int ax = 0; ax < 3; ax++) {
    ctx->qlo[ax] = HUGE_VAL;
    ctx->qhi[ax] = -HUGE_VAL;
    for (int i = 0; i < nc; i++) {
      ctx->qlo[ax] = std::min(ctx->qlo[ax], qlo[i][ax]);
      ctx->qhi[ax] = std::max(ctx->qhi[ax], qhi[i][ax]);
    }
  }
  if (n) {
    PMX_CK(C, hipMemcpyAsync(ctx->d_qxyz.p, hx, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (tg) PMX_CK(C, hipMemcpyAsync(ctx->d_qtag.p, htg, (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream));
  }
  tr.mark("coords");
  ctx->nq = n;
  if (!pmx_dgrow(ctx, ctx->d_wmask, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_elem, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_status, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_steps, nn)) return 0;
  // points a step never locates (NUL, frozen, orphans) report element 0
  PMX_CK(C, hipMemsetAsync(ctx->d_elem.p, 0, nn * sizeof(int), ctx->stream));
  PMX_CK(C, hipMemsetAsync(ctx->d_status.p, 0, nn * sizeof(int), ctx->stream));
  PMX_CK(C, hipMemsetAsync(ctx->d_steps.p, 0, nn * sizeof(int), ctx->stream));
  if (!pmx_dgrow(ctx, ctx->d_start, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_edge, nn)) return 0;
  if (!pmx_dgrow(ctx, ctx->d_vertex, nn)) return 0;
  // start 0, edge / vertex unset (-1) for every point no step writes
  PMX_CK(C, hipMemsetAsync(ctx->d_start.p, 0, nn * sizeof(int), ctx->stream));
  PMX_CK(C, hipMemsetAsync(ctx->d_edge.p, 0xff, nn * sizeof(int), ctx->stream));
  PMX_CK(C, hipMemsetAsync(ctx->d_vertex.p, 0xff, nn * sizeof(int), ctx->stream));
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
  ctx->ntets.view_kept(*pv, ntet);
  return 1;
}

// The new points' source vertices (MMG5_Point.src of a USE_POINTMAP build),
// packed dense in the pinned arena and sent on the context's stream.  Any int
// is accepted: a source outside 1..np of the step's background, or one no
// element holds, starts its walk from element 1 (resolved on the device).
int pmx_upload_point_sources(pmx_ctx *ctx, const int *src, int64_t stride) {
  if (!ctx) return 0;
  const pmx_call C{ctx};
  if (!ctx->have_pts) return C.fail("pmx_upload_point_sources: upload the points first");
  ctx->have_src = false;
  if (!src) return 1;
  if (stride < (int64_t)sizeof(int)) return C.fail("pmx_upload_point_sources: bad stride");
  (void)hipSetDevice(ctx->device);
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
    PMX_CK(C, hipMemcpyAsync(ctx->d_qsrc.p, h, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  }
  ctx->have_src = true;
  return 1;
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
  const pmx_call C{ctx};
  if (!ctx->have_pts) return C.fail("pmx_upload_new_tets: upload the new points first");
  if (!tetra_v || ne < 1 || tetra_stride < 16 || 4 * ne >= (1LL << 31)) return C.fail("pmx_upload_new_tets: bad new tets");
  (void)hipSetDevice(ctx->device);
  return ctx->ntets.replace(tetra_v, tetra_stride, ne) ? 1 : 0;
}

}  // extern "C"

// the new points' classification and compaction on stream s (the marks, if
// any, zeroed beforehand)
bool pmx_ctx::classify(hipStream_t s, bool marks, bool pointmap) {
  if (nq < 1) return true;
  const uint16_t *tg = have_qtag ? d_qtag.p : nullptr;
  const uint8_t *mk = marks ? ntets.d_mark.p : nullptr;
  if (pointmap) {
    const PointMapArgs pma{d_qsrc.p, d_pmap.p, d_pmap.p + (np + 1), np, d_pstart.p, d_pstart.p + nq};
    launch_classify_pointmap(tg, mk, nq, d_ctile.p, d_kind.p, d_vollist.p, d_bdylist.p, d_nsel.p, pma, s);
  } else {
    launch_classify(tg, mk, nq, d_ctile.p, d_kind.p, d_vollist.p, d_bdylist.p, d_nsel.p, s);
  }
  return pmx_call{this}.ok(hipGetLastError(), "classification: launch failed");
}
