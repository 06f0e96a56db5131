// pmx_points.hip -- the new points and the new tets, host side and kernels.
//
// pmx_upload_points / pmx_upload_point_sources, the points' classification,
// and NewTets: the new mesh's tets on the device with the orphan reset that
// depends on them.  Every assignment to a NewTets member is in this file; its
// states and transitions are the table at the struct (pmx_internal.h).
//
// k_mark_new_tets,   the orphan marks: the points some valid new tet holds
// k_mark_new_tets_win  (plain byte stores / deduplicated in an LDS window)
// k_orphans          the rows of the unmarked points back to "never visited"
// k_cls_count,       the points' kinds and their order-preserving compaction
// k_cls_write        into the volume / surface lists (PM: with the start
//                    elements of a PMX_RUN_POINTMAP step)
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

// the orphan marks from the new tets on the device: point j (0-based) is
// marked when a valid new tet (1-based vertex j + 1) holds it -- the
// reference's vertex loop over the new tets (src/interpmesh_pmmg.c:535-541).
// HBM-bound on the 16-B tet reads; the byte stores are what costs beyond
// them (r06: 0.50 ms at C3 with four stores per tet), so a lane skips the
// vertices its left neighbour -- the previous tet, which in any coherent
// numbering shares most of them -- also holds (that lane stores them), and
// each lane takes two tets per round (two loads in flight).
// H tets per thread and iteration (loads in flight)
template <int H>
__global__ __launch_bounds__(256) void k_mark_new_tets(const int4 *__restrict__ tv, int64_t ne,
                                                       uint8_t *__restrict__ mk) {
  // (r06: an XCD-aware split -- each XCD one contiguous eighth of the tets,
  // so its byte stores stay in its own L2 -- measured 0.565 vs 0.549 ms
  // beside the step's prefix: not kept)
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  const int64_t nit = (ne + H * st - 1) / (H * st);    // uniform trip count (the shuffles below)
  const bool lane0 = (threadIdx.x & 63) == 0;
  for (int64_t it = 0; it < nit; it++) {
    const int64_t k0 = 1 + H * (it * st + (int64_t)blockIdx.x * blockDim.x) + threadIdx.x;
    int4 v[H];
#pragma unroll
    for (int h = 0; h < H; h++) {
      const int64_t k = k0 + h * blockDim.x;
      v[h] = k <= ne ? tv[k] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (int h = 0; h < H; h++) {
      const int4 a = v[h];
      int4 u;
      u.x = __shfl_up(a.x, 1, 64); u.y = __shfl_up(a.y, 1, 64);
      u.z = __shfl_up(a.z, 1, 64); u.w = __shfl_up(a.w, 1, 64);
      if (lane0 || u.x <= 0) u = make_int4(0, 0, 0, 0);   // no valid left neighbour: store all
      if (a.x <= 0) continue;                             // !MG_EOK
      const int w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const int q = w[l];
        if (q != u.x && q != u.y && q != u.z && q != u.w) mk[q - 1] = 1;
      }
    }
  }
}
// r06 (late): the marks deduplicated in LDS.  What bounds k_mark_new_tets is
// not its 16-B tet stream but its byte stores: one L2 write request per lane
// and vertex (≈ 1.5-2 per tet after the left-neighbour filter, a vertex is in
// ≈ 24 tets).  Here a workgroup takes 256 H consecutive tets at a time and
// marks their vertices in an LDS byte window [wb, wb + MW_WIN) anchored at
// the chunk's first valid tet (a coherent numbering -- Morton or Scotch --
// keeps a chunk's vertices together); the window is flushed as 32-bit words,
// one global atomicOr per word that holds a mark (the bytes of the marks
// array ORed: marks are only ever set, so concurrent chunks and the plain
// byte stores of out-of-window vertices compose).  Any numbering stays
// correct: a vertex outside the window is stored directly, as before.
#define MW_WIN 16384
template <int H>
__global__ __launch_bounds__(256) void k_mark_new_tets_win(const int4 *__restrict__ tv, int64_t ne,
                                                           uint8_t *__restrict__ mk, int64_t nmk) {
  __shared__ unsigned win[MW_WIN / 4];
  __shared__ int s_base;
  unsigned *mk32 = reinterpret_cast<unsigned *>(mk);
  uint8_t *wb8 = reinterpret_cast<uint8_t *>(win);
  for (int i = threadIdx.x; i < MW_WIN / 4; i += 256) win[i] = 0u;
  const int64_t C = 256 * H;
  const int64_t nch = (ne + C - 1) / C;
  const bool lane0 = (threadIdx.x & 63) == 0;
  for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {        // uniform over the workgroup
    const int64_t k0 = 1 + c * C + threadIdx.x;
    int4 v[H];
#pragma unroll
    for (int h = 0; h < H; h++) {
      const int64_t k = k0 + h * 256;
      v[h] = k <= ne ? tv[k] : make_int4(0, 0, 0, 0);
    }
    // window anchor: the first valid tet's smallest vertex, less a quarter
    // window (vertices of a chunk's later cells may precede it), 4-aligned
    if (threadIdx.x == 0) {
      const int4 a = v[0];
      const int m = a.x > 0 ? min(min(a.x, a.y), min(a.z, a.w)) - 1 : 0;
      s_base = max(0, m - MW_WIN / 4) & ~3;
    }
    __syncthreads();
    const int wb = s_base;
#pragma unroll
    for (int h = 0; h < H; h++) {
      const int4 a = v[h];
      int4 u;
      u.x = __shfl_up(a.x, 1, 64); u.y = __shfl_up(a.y, 1, 64);
      u.z = __shfl_up(a.z, 1, 64); u.w = __shfl_up(a.w, 1, 64);
      if (lane0 || u.x <= 0) u = make_int4(0, 0, 0, 0);
      if (a.x <= 0) continue;                             // !MG_EOK
      const int w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const int q = w[l];
        if (q == u.x || q == u.y || q == u.z || q == u.w) continue;
        const unsigned off = (unsigned)(q - 1 - wb);
        if (off < (unsigned)MW_WIN) wb8[off] = 1;
        else mk[q - 1] = 1;
      }
    }
    __syncthreads();
    // flush: one atomicOr per word holding a mark, then clear it
    const int64_t w0 = wb >> 2;
    for (int i = threadIdx.x; i < MW_WIN / 4; i += 256) {
      const unsigned x = win[i];
      if (x) {
        if (w0 + i < (nmk + 3) / 4) atomicOr(mk32 + w0 + i, x);
        win[i] = 0u;
      }
    }
    __syncthreads();
  }
}

// the window kernel when the sizes allow (its word flush indexes in 32 bits),
// else the plain marks
static void launch_mark_new_tets(const int4 *tv, int64_t ne, uint8_t *mk, int64_t nmk, hipStream_t s) {
  if (ne < 1) return;
  if (nmk > 0 && nmk < INT32_MAX - MW_WIN) {
    hipLaunchKernelGGL(k_mark_new_tets_win<4>, dim3(pmx_grid(ne, 4096, 256 * 4)), dim3(256), 0, s, tv, ne, mk, nmk);
    return;
  }
  hipLaunchKernelGGL(k_mark_new_tets<2>, dim3(pmx_grid(ne, 8192, 256 * 2)), dim3(256), 0, s, tv, ne, mk);
}

// the rows of points in no valid new tet, after a step that located them:
// back to untouched (the constant-size bit kept), element / status / steps /
// start 0, edge / vertex unset (-1), and their kind KIND_ORPH, so that the
// locate statistics count only the points the reference visits (a NUL or
// frozen point keeps its kind: the step never located it)
struct OrphanRows {
  uint8_t *wmask;
  int *elem, *status, *steps, *start, *edge, *vertex;
  int8_t *kind;
};
__global__ __launch_bounds__(256) void k_orphans(const uint8_t *__restrict__ mk, int64_t n, uint8_t keep,
                                                 OrphanRows r) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    if (mk[j]) continue;
    r.wmask[j] &= keep;
    r.elem[j] = 0;
    r.status[j] = 0;
    r.steps[j] = 0;
    r.start[j] = 0;
    r.edge[j] = -1;
    r.vertex[j] = -1;
    const int8_t k = r.kind[j];
    if (k == KIND_VOL || k == KIND_BDY) r.kind[j] = KIND_ORPH;
  }
}
// points in no valid new tet (mk == 0) after a step: rows back to untouched
static void launch_orphans(const uint8_t *mk, int64_t n, uint8_t keep, const OrphanRows &r, hipStream_t s) {
  if (n < 1) return;
  hipLaunchKernelGGL(k_orphans, dim3(pmx_grid(n, 4096)), dim3(256), 0, s, mk, n, keep, r);
}

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

// ---- new points: classification on the device (pmx_upload_points) ---------------

// new points, every step (the tag dispatch of the reference's vertex loop,
// src/interpmesh_pmmg.c:541-560): kinds (mark != NULL: the orphan marks of
// the new tets, 0 = in no valid new tet) and the order-preserving compaction into
// the volume / surface lists; counts into nsel[0..1].  tcnt: scratch of cls_tiles(n) int2.
#define CLS_TILE 16384               // 4 rounds of 256 threads x 16 points
static inline int64_t cls_tiles(int64_t n) { return (n + CLS_TILE - 1) / CLS_TILE; }

// sum over the 256-thread block, in every thread (red: 4 LDS slots)
__device__ __forceinline__ int2 block_sum2(int2 v, int2 *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v.x += __shfl_xor(v.x, o, 64);
    v.y += __shfl_xor(v.y, o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int2 r = red[0];
#pragma unroll
  for (int w = 1; w < 4; w++) { r.x += red[w].x; r.y += red[w].y; }
  return r;
}

// The kinds of the 16 points j0 .. j0+15 of one thread (j0 % 16 == 0): two
// 16-B tag loads and one 16-B mark load instead of 16 narrow loads per lane
// (r03: the one-point-per-lane rounds were latency-bound, 0.12 ms at C3 for
// 17 M points); points at or past n get 0xff.  kw: the kinds, 4 per word.
__device__ __forceinline__ void kinds16(const uint16_t *__restrict__ tag, const uint8_t *__restrict__ mark,
                                        int64_t j0, int64_t n, unsigned kw[4], int &cv, int &cb) {
  unsigned tw[8], mw[4];
  if (j0 + 16 <= n) {
    if (tag) {
      const uint4 a = reinterpret_cast<const uint4 *>(tag + j0)[0];
      const uint4 b = reinterpret_cast<const uint4 *>(tag + j0)[1];
      tw[0] = a.x; tw[1] = a.y; tw[2] = a.z; tw[3] = a.w;
      tw[4] = b.x; tw[5] = b.y; tw[6] = b.z; tw[7] = b.w;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) tw[i] = 0u;
    }
    if (mark) {
      const uint4 c = *reinterpret_cast<const uint4 *>(mark + j0);
      mw[0] = c.x; mw[1] = c.y; mw[2] = c.z; mw[3] = c.w;
    }
  } else {                                    // the last, partial chunk
#pragma unroll
    for (int i = 0; i < 8; i++) tw[i] = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) mw[i] = 0u;
    for (int i = 0; i < 16 && j0 + i < n; i++) {
      if (tag) tw[i >> 1] |= (unsigned)tag[j0 + i] << (16 * (i & 1));
      if (mark) mw[i >> 2] |= (unsigned)mark[j0 + i] << (8 * (i & 3));
    }
  }
#pragma unroll
  for (int w = 0; w < 4; w++) kw[w] = 0u;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const unsigned t = (tw[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    const bool in = j0 + i < n;
    // kind of a new point: PMMG_interpMetricsAndFields_mesh's dispatch
    // (src/interpmesh_pmmg.c:541-560): !MG_VOK, MG_REQ (copied by
    // PMMG_copyMetricsAndFields_point over every point, :311-446, whatever
    // the tets), in no valid new tet (never visited), MG_BDY, volume
    unsigned k = (t >= PMX_TAG_NUL) ? KIND_NUL
                 : (t & PMX_TAG_REQ) ? KIND_SKIP
                 : (mark && !((mw[i >> 2] >> (8 * (i & 3))) & 0xffu)) ? KIND_ORPH
                 : (t & PMX_TAG_BDY) ? KIND_BDY : KIND_VOL;
    k = in ? k : 0xffu;
    cv += k == KIND_VOL;
    cb += k == KIND_BDY;
    kw[i >> 2] |= k << (8 * (i & 3));
  }
}

// per tile of CLS_TILE points: how many volume / surface points
__global__ __launch_bounds__(256) void k_cls_count(const uint16_t *__restrict__ tag, const uint8_t *__restrict__ mark,
                                                   int64_t n, int2 *__restrict__ tcnt) {
  __shared__ int2 red[4];
  const int64_t t0 = (int64_t)blockIdx.x * CLS_TILE;
  int cv = 0, cb = 0;
#pragma unroll
  for (int r = 0; r < CLS_TILE / 4096; r++) {
    const int64_t j0 = t0 + r * 4096 + 16 * (int64_t)threadIdx.x;
    unsigned kw[4];
    if (j0 < n) kinds16(tag, mark, j0, n, kw, cv, cb);
  }
  const int2 c = block_sum2(make_int2(cv, cb), red);
  if (threadIdx.x == 0) tcnt[blockIdx.x] = c;
}

// launch_classify that also carries the source vertices src[0..n) through the
// compaction: vstart[j] / bstart[j] = the start element of the j-th volume /
// surface point, vmap / tmap of its source, 1 when the source is outside
// 1..np or no element holds it
struct PointMapArgs {
  const int *src;
  const unsigned *vmap, *tmap;
  int64_t np;
  int *vstart, *bstart;
};

// kinds + the two lists in input order.  Per round of 4096 points: every
// thread classifies 16 consecutive points (vector loads, one 16-B kind
// store) into LDS; wave w owns points 1024 w .. 1024 w + 1023 of the round
// (its own threads' chunks), so the wave totals give each wave its base, and
// the wave then writes its list entries in 16 coalesced ballot sub-rounds.
// Tile base = sum of the previous tiles' counts, summed again by every
// workgroup (a few KB of L2 reads instead of a third launch).
// PM (PMX_RUN_POINTMAP): the point's source vertex goes through the
// compaction with it -- the start element of list entry j is resolved here
// (one coalesced read of the sources, one gather of the map), so that the
// walks read a coalesced int.
// (The point-map arguments are a parameter pack: empty for the default
// kernel, whose argument block and code stay what they were.)
__device__ __forceinline__ const PointMapArgs &cls_pm(const PointMapArgs &a) { return a; }
template <bool PM, class... PMA>
__global__ __launch_bounds__(256) void k_cls_write(const uint16_t *__restrict__ tag,
                                                   const uint8_t *__restrict__ mark, int64_t n,
                                                   const int2 *__restrict__ tcnt, int8_t *__restrict__ kind,
                                                   int *__restrict__ vlist, int *__restrict__ blist,
                                                   int *__restrict__ nsel, PMA... pma) {
  __shared__ int2 red[4];
  __shared__ int2 wc[4];
  __shared__ uint4 lk[256];                   // the round's 4096 kinds
  int pv = 0, pb = 0;
  for (unsigned t = threadIdx.x; t < blockIdx.x; t += 256) {
    const int2 c = tcnt[t];
    pv += c.x;
    pb += c.y;
  }
  int2 base = block_sum2(make_int2(pv, pb), red);
  const int64_t t0 = (int64_t)blockIdx.x * CLS_TILE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint8_t *lkb = reinterpret_cast<const uint8_t *>(lk);
  for (int r = 0; r < CLS_TILE / 4096; r++) {
    const int64_t r0 = t0 + r * 4096;
    if (r0 >= n) break;                                   // uniform: the tile's end
    const int64_t j0 = r0 + 16 * (int64_t)threadIdx.x;
    unsigned kw[4] = {~0u, ~0u, ~0u, ~0u};
    int cv = 0, cb = 0;
    if (j0 < n) {
      kinds16(tag, mark, j0, n, kw, cv, cb);
      if (j0 + 16 <= n) *reinterpret_cast<uint4 *>(kind + j0) = make_uint4(kw[0], kw[1], kw[2], kw[3]);
      else
        for (int i = 0; j0 + i < n; i++) kind[j0 + i] = (int8_t)((kw[i >> 2] >> (8 * (i & 3))) & 0xffu);
    }
    lk[threadIdx.x] = make_uint4(kw[0], kw[1], kw[2], kw[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cv += __shfl_xor(cv, o, 64);
      cb += __shfl_xor(cb, o, 64);
    }
    if (lane == 0) wc[w] = make_int2(cv, cb);
    __syncthreads();
    int ov = base.x, ob = base.y;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int2 c = wc[q];
      ov += q < w ? c.x : 0;
      ob += q < w ? c.y : 0;
      base.x += c.x;
      base.y += c.y;
    }
    // the wave's 1024 points in input order, 64 per sub-round
#pragma unroll 4
    for (int s = 0; s < 16; s++) {
      const int p = 1024 * w + 64 * s + lane;
      const int k = lkb[p];
      const unsigned long long bv = __ballot(k == KIND_VOL), bb = __ballot(k == KIND_BDY);
      if (k == KIND_VOL) vlist[ov + __popcll(bv & below)] = (int)(r0 + p);
      else if (k == KIND_BDY) blist[ob + __popcll(bb & below)] = (int)(r0 + p);
      if constexpr (PM) {
        const PointMapArgs &pm = cls_pm(pma...);
        if (k == KIND_VOL || k == KIND_BDY) {
          const int sv = pm.src[r0 + p];
          unsigned e = 0xffffffffu;
          if (sv >= 1 && (int64_t)sv <= pm.np) e = (k == KIND_VOL ? pm.vmap : pm.tmap)[sv];
          const int st = e == 0xffffffffu ? 1 : (int)e;     // the reference's initial start
          if (k == KIND_VOL) pm.vstart[ov + __popcll(bv & below)] = st;
          else pm.bstart[ob + __popcll(bb & below)] = st;
        }
      }
      ov += __popcll(bv);
      ob += __popcll(bb);
    }
    __syncthreads();                                      // lk and wc rewritten next round
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    nsel[0] = base.x;
    nsel[1] = base.y;
  }
}

static void launch_classify(const uint16_t *tag, const uint8_t *mk, int64_t n, int2 *tcnt, int8_t *kind, int *vlist,
                            int *blist, int *nsel, hipStream_t s) {
  if (n < 1) return;
  const unsigned nt = (unsigned)cls_tiles(n);
  hipLaunchKernelGGL(k_cls_count, dim3(nt), dim3(256), 0, s, tag, mk, n, tcnt);
  hipLaunchKernelGGL((k_cls_write<false>), dim3(nt), dim3(256), 0, s, tag, mk, n, (const int2 *)tcnt, kind, vlist,
                     blist, nsel);
}
static void launch_classify_pointmap(const uint16_t *tag, const uint8_t *mk, int64_t n, int2 *tcnt, int8_t *kind,
                                     int *vlist, int *blist, int *nsel, const PointMapArgs &pm, hipStream_t s) {
  if (n < 1) return;
  const unsigned nt = (unsigned)cls_tiles(n);
  hipLaunchKernelGGL(k_cls_count, dim3(nt), dim3(256), 0, s, tag, mk, n, tcnt);
  hipLaunchKernelGGL((k_cls_write<true, PointMapArgs>), dim3(nt), dim3(256), 0, s, tag, mk, n, (const int2 *)tcnt,
                     kind, vlist, blist, nsel, pm);
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
