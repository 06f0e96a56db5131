// pmx_more.hip -- pmx_interp_more: further solution fields of the uploaded
// background onto the points the last step located, without a second walk.
//
// The located element and the barycentrics of a point depend on the point and
// the background only, never on the fields (PMMG_interpMetricsAndFields_mesh
// locates once and loops `for j < mesh->nsols`, reference
// src/interpmesh_pmmg.c:578-595, :619-636).  The fused step carries at most
// PMX_MAX_SOLS solutions (SolDesc, the 8-bit write mask, the row width of
// k_walks); any number beyond them is interpolated here in batches of
// PMX_MAX_SOLS from the step's results:
//  * volume points: the barycentrics are recomputed from (elem, status, p)
//    with the step's own device functions -- the reference quotients of
//    PMMG_locatePointInTetra (tet_lambda) for status +-1, the one-hot of
//    PMMG_barycoord3d_getClosest for status 0 -- the same operations under
//    -ffp-contract=off, hence the same bits; nothing is stored per point;
//  * surface points: the walk's barycoord array is not a function of
//    (tria, p) alone (a shadow-wedge hit rewrites it, the exhaustive not-found
//    branch evaluates it on another tria's geometry), so the step (interp_tria) keeps it
//    per entry of the surface list (d_bphi, 32 B) and this path reads it back;
//    fields always go through PMMG_interp3bar_{iso,ani} (only the metric is
//    copied at a vertex or interpolated along an edge, and it stays in the step).
// One thread per entry of the step's compacted lists, no dependent walk chain:
// bandwidth-bound gathers of the tet record, 4 vertices and 4 batch rows.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>

#include "pmx_internal.h"

struct MoreArgs {
  const double *xyz;            // old vertices, 24 B
  const TetRec *tets;
  const TriRec *tris;
  int64_t ne, nt;
  const double *sol;            // the batch's background rows, [np + 1][sd.S]
  SolDesc sd;                   // the batch's layout (no metric)
  const double *q;              // new points, dense x y z
  const int8_t *kind;           // the step's kinds (an orphan reset makes a point KIND_ORPH)
  const int *elem, *status;     // the step's results
  const Pt4 *bphi;              // surface points: the step's barycentrics, per surface-list entry
  const int *list;              // the step's compacted list (volume or surface)
  const int *nlist_dev;
  double *out;                  // [nq][sd.S]
  uint8_t *wmask;               // [nq], zeroed before the launch
};

template <int LAYOUT, int S>
__global__ __launch_bounds__(256) void k_more_vol(MoreArgs A) {
  // the walk's block order: each XCD's L2 sees a contiguous range of points
  const int64_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t j = b * blockDim.x + threadIdx.x;
  if (j >= *A.nlist_dev) return;
  const int64_t i = A.list[j];
  if (A.kind[i] != KIND_VOL) return;                 // an orphan, reset since the step
  const int k = A.elem[i];
  if (k <= 0 || k > A.ne) return;                    // no tet at all: untouched
  const int st = A.status[i];
  const TetRec t = A.tets[k];
  if (t.v[0] <= 0) return;
  const D3 p{A.q[3 * i], A.q[3 * i + 1], A.q[3 * i + 2]};
  const int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
  const D3 P[4] = {ld3(A.xyz, v[0]), ld3(A.xyz, v[1]), ld3(A.xyz, v[2]), ld3(A.xyz, v[3])};
  double lam[4];
  if (st != 0) {
    // found by a walk, the tie rule or the exhaustive scan: the reference's quotients
    double vol;
    tet_lambda(P, p, lam, &vol);
  } else {
    // closest tet: PMMG_barycoord3d_getClosest, nearest vertex, first on ties
    double best = 0.0;
    int it = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const double d0 = p.x - P[l].x, d1 = p.y - P[l].y, d2 = p.z - P[l].z;
      const double d = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      if (l == 0 || d < best) { best = d; it = l; }
    }
#pragma unroll
    for (int l = 0; l < 4; l++) lam[l] = (l == it) ? 1.0 : 0.0;
  }
  const unsigned wm = interp_layout<LAYOUT, S>(A.sol, A.sd, v, lam, A.out + i * A.sd.S);
  A.wmask[i] = (uint8_t)wm;
}

__global__ __launch_bounds__(256) void k_more_bdy(MoreArgs A) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= *A.nlist_dev) return;
  const int64_t i = A.list[j];
  if (A.kind[i] != KIND_BDY) return;
  const int k = A.elem[i];
  if (k <= 0 || k > A.nt) return;
  const TriRec t = A.tris[k];
  if (t.v[0] <= 0) return;
  const Pt4 b = A.bphi[j];
  const int v[3] = {t.v[0], t.v[1], t.v[2]};
  const double phi[3] = {b.x, b.y, b.z};
  // PMMG_interp3bar_iso / _ani (src/interpmesh_pmmg.c:125-190), as interp_tria
  // applies them to every solution that is not the metric
  const unsigned wm = interp_bar<3>(A.sol, A.sd, v, phi, A.out + i * A.sd.S);
  A.wmask[i] = (uint8_t)wm;
}

template <int LAYOUT, int S> static void launch_more_vol_t(const MoreArgs &a, int64_t nb, hipStream_t s) {
  hipLaunchKernelGGL((k_more_vol<LAYOUT, S>), dim3((unsigned)nb), dim3(256), 0, s, a);
}

// the batch layout, as walk_layout without a metric: all scalars / vectors
// with 1..8 doubles per row -> LAYOUT_ISO (16-B loads for an even row), else
// the generic interp_bar<4>
static void launch_more_vol(const MoreArgs &a, int64_t nlist_ub, hipStream_t s) {
  const int64_t nb = (nlist_ub + 255) / 256;
  if (nb < 1) return;
  bool iso = a.sd.S >= 1 && a.sd.S <= 8;
  for (int k = 0; k < a.sd.nsol; k++) iso = iso && a.sd.size[k] != 6;
  if (iso) {
    switch (a.sd.S) {
      case 1: return launch_more_vol_t<LAYOUT_ISO, 1>(a, nb, s);
      case 2: return launch_more_vol_t<LAYOUT_ISO, 2>(a, nb, s);
      case 3: return launch_more_vol_t<LAYOUT_ISO, 3>(a, nb, s);
      case 4: return launch_more_vol_t<LAYOUT_ISO, 4>(a, nb, s);
      case 5: return launch_more_vol_t<LAYOUT_ISO, 5>(a, nb, s);
      case 6: return launch_more_vol_t<LAYOUT_ISO, 6>(a, nb, s);
      case 7: return launch_more_vol_t<LAYOUT_ISO, 7>(a, nb, s);
      default: return launch_more_vol_t<LAYOUT_ISO, 8>(a, nb, s);
    }
  }
  launch_more_vol_t<LAYOUT_GEN, 0>(a, nb, s);
}

static void launch_more_bdy(const MoreArgs &a, int64_t nlist_ub, hipStream_t s) {
  const int64_t nb = (nlist_ub + 255) / 256;
  if (nb < 1) return;
  hipLaunchKernelGGL(k_more_bdy, dim3((unsigned)nb), dim3(256), 0, s, a);
}

#define CK(x) PMX_CK(C, x)

double pmx_more_kernel_ms(pmx_ctx *ctx) {
  if (ctx->more_ev_used == 0) return -1.0;
  hipStreamSynchronize(ctx->stream);
  double tot = 0.0;
  for (int b = 0; b < ctx->more_ev_used; b++) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, ctx->more_ev[2 * (size_t)b], ctx->more_ev[2 * (size_t)b + 1]);
    tot += ms;
  }
  return tot;
}

extern "C" int pmx_interp_more(pmx_ctx *ctx, int nsol, const pmx_sol_view *old_sols, const pmx_sol_view *new_sols,
                               int64_t npts_cap) {
  if (!ctx) return 0;
  if (!ctx->stepped() || !ctx->have_bg) {
    ctx->err = "pmx_interp_more: no step has run on the current uploads";
    return 0;
  }
  if (!ctx->located) {
    ctx->err = "pmx_interp_more: the last step had nothing to interpolate and located no point";
    return 0;
  }
  if (nsol < 1 || !old_sols || !new_sols) { ctx->err = "pmx_interp_more: bad field list"; return 0; }
  for (int k = 0; k < nsol; k++) {
    const int sz = old_sols[k].size;
    if ((sz != 1 && sz != 3 && sz != 6) || !old_sols[k].m || new_sols[k].size != sz) {
      ctx->err = "pmx_interp_more: null or mismatched solution";
      return 0;
    }
  }
  if (npts_cap < ctx->nq) {
    ctx->err = "pmx_interp_more: output capacity " + std::to_string(npts_cap) + " < " + std::to_string(ctx->nq) +
               " entries needed";
    return 0;
  }
  hipSetDevice(ctx->device);
  const pmx_call C{ctx, "pmx_interp_more", ctx->stream};
  ctx->more_ev_used = 0;
  // the orphans' rows first, as every consumer of the step's results
  if (!ctx->ntets.fix_orphans()) return 0;
  const int64_t n = ctx->nq, np = ctx->np;
  if (n == 0) {
    CK(hipStreamSynchronize(ctx->stream));
    return ctx->check_device_errors() ? 1 : 0;
  }
  hipStream_t s = ctx->stream;
  const int nbatch = (nsol + PMX_MAX_SOLS - 1) / PMX_MAX_SOLS;
  if (ctx->more_ev.size() < 2 * (size_t)nbatch) ctx->more_ev.resize(2 * (size_t)nbatch);
  for (auto &e : ctx->more_ev)
    if (!e.create()) return C.fail("event");
  for (int b = 0; b < nbatch; b++) {
    const int k0 = b * PMX_MAX_SOLS, nb = std::min(PMX_MAX_SOLS, nsol - k0);
    SolDesc sd{};
    sd.nsol = nb;
    sd.imet = -1;
    int S = 0;
    for (int k = 0; k < nb; k++) {
      sd.size[k] = old_sols[k0 + k].size;
      sd.off[k] = S;
      S += sd.size[k];
    }
    sd.S = S;
    const size_t in_n = (size_t)(np + 1) * S, out_n = (size_t)n * S;
    if (!pmx_dgrow(ctx, ctx->d_msol, in_n) || !pmx_dgrow(ctx, ctx->d_mout, out_n) ||
        !pmx_dgrow(ctx, ctx->d_mwm, (size_t)n))
      return 0;
    // pinned arena: packed background rows | output rows | write masks (handed
    // out once the stream has drained: the previous batch is done with it)
    const size_t o_in = 0, o_out = o_in + pmx_call::al256(in_n * sizeof(double)),
                 o_wm = o_out + pmx_call::al256(out_n * sizeof(double)), total = o_wm + pmx_call::al256((size_t)n);
    char *stg = pmx_hstage(ctx, total);
    if (!stg) return 0;
    double *hs = (double *)(stg + o_in);
    // interleaved [np + 1][S] as pmx_upload_background packs them, in blocks
    // of 1024 rows (each row's line written while it is in cache)
    pmx_par_for(0, np + 1, [&](int64_t i0, int64_t i1) {
      for (int64_t b0 = i0; b0 < i1; b0 += 1024) {
        const int64_t b1 = std::min(i1, b0 + 1024);
        for (int k = 0; k < nb; k++) {
          const int sz = sd.size[k], off = sd.off[k];
          const double *src = old_sols[k0 + k].m;
          for (int64_t i = b0; i < b1; i++)
            for (int j = 0; j < sz; j++) hs[(size_t)i * S + off + j] = src[i * sz + j];
        }
      }
    });
    CK(hipMemcpyAsync(ctx->d_msol.p, hs, in_n * sizeof(double), hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(ctx->d_mwm.p, 0, (size_t)n, s));
    MoreArgs A{};
    A.xyz = ctx->d_xyz.p; A.tets = ctx->d_tets.p; A.tris = ctx->d_tris.p; A.ne = ctx->ne; A.nt = ctx->nt;
    A.sol = ctx->d_msol.p; A.sd = sd; A.q = ctx->d_qxyz.p; A.kind = ctx->d_kind.p;
    A.elem = ctx->d_elem.p; A.status = ctx->d_status.p; A.bphi = ctx->d_bphi.p;
    A.out = ctx->d_mout.p; A.wmask = ctx->d_mwm.p;
    CK(hipEventRecord(ctx->more_ev[2 * (size_t)b], s));
    if (ctx->nq_vol_ub > 0) {
      A.list = ctx->d_vollist.p; A.nlist_dev = ctx->d_nsel.p;
      launch_more_vol(A, ctx->nq_vol_ub, s);
    }
    if (ctx->nq_bdy_ub > 0 && ctx->nt > 0 && ctx->d_bphi.p) {
      A.list = ctx->d_bdylist.p; A.nlist_dev = ctx->d_nsel.p + 1;
      launch_more_bdy(A, ctx->nq_bdy_ub, s);
    }
    CK(hipEventRecord(ctx->more_ev[2 * (size_t)b + 1], s));
    ctx->more_ev_used = b + 1;
    CK(hipGetLastError());
    const double *ho = (const double *)(stg + o_out);
    const uint8_t *wm = (const uint8_t *)(stg + o_wm);
    CK(hipMemcpyAsync(stg + o_out, ctx->d_mout.p, out_n * sizeof(double), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(stg + o_wm, ctx->d_mwm.p, (size_t)n, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (b == 0 && !ctx->check_device_errors()) return 0;   // the step's own error word
    // rows the reference leaves alone (no mask bit) are not written
    pmx_par_for(0, n, [&](int64_t i0, int64_t i1) {
      for (int64_t b0 = i0; b0 < i1; b0 += 1024) {
        const int64_t b1 = std::min(i1, b0 + 1024);
        for (int k = 0; k < nb; k++) {
          double *dst = new_sols[k0 + k].m;
          if (!dst) continue;
          const int sz = sd.size[k], off = sd.off[k];
          const unsigned bit = 1u << k;
          for (int64_t i = b0; i < b1; i++) {
            if (!(wm[i] & bit)) continue;
            memcpy(dst + i * sz, ho + (size_t)i * S + off, sizeof(double) * (size_t)sz);
          }
        }
      }
    });
  }
  return 1;
}
