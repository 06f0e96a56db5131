// pmx_graph.hip -- the Metis element graph and its edge weights on gfx950.
//
// pmx_metis_graph / pmx_face_weights <- PMMG_graph_meshElts2metis and
//                         PMMG_computeWgt (reference src/metis_pmmg.c:746-823,
//                         280-301): load balancing's element graph and its
//                         edge weights
//
// The graph of the uploaded group, tets as Metis nodes: xadj / adjncy from the
// records' neighbours in (k, f) order (a count, an inclusive scan, a fill),
// and PMMG_computeWgt per interior face as the edge weight.  MMG5_iarf and the
// MMG5_lenedg dispatch (iso: MMG5_lenedg_iso; tensor: MMG5_lenedg33_ani, or
// MMG5_lenedg_ani with metRidTyp = 1) are restated from Mmg's public sources,
// unpinned, as for k_prilen: the same device functions (pmx_metric.h) give the
// lengths.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string>
#include "pmx_internal.h"
#include "pmx_metric.h"

#define PMX_WGT_HUGE 1000000.0     // PMMG_WGTVAL_HUGEINT

// degrees: deg[0] = 0, deg[k] = the interior faces of tet k -- their inclusive
// sum is xadj[0..ne].  A deleted tet (the reference wants a packed mesh)
// raises *flag.
__global__ __launch_bounds__(256) void k_graph_count(const TetRec *__restrict__ tets, int64_t ne,
                                                     int *__restrict__ deg, unsigned *__restrict__ flag) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > ne) return;
  if (k == 0) { deg[0] = 0; return; }
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  const int4 v = recs[2 * k], nb = recs[2 * k + 1];
  if (v.x <= 0) *flag = 1u;
  deg[k] = (nb.x != 0) + (nb.y != 0) + (nb.z != 0) + (nb.w != 0);
}

// one term of PMMG_computeWgt's sum
__device__ __forceinline__ double wgt_term(double len) { return len <= 1.0 ? len - 1.0 : 1.0 / len - 1.0; }
// ... and its end: MG_MIN(1.0 / exp(alpha * res / 3.0), PMMG_WGTVAL_HUGEINT), alpha = 28
__device__ __forceinline__ double wgt_of(double res) {
  const double w = 1.0 / exp(28.0 * res / 3.0);
  return w < PMX_WGT_HUGE ? w : PMX_WGT_HUGE;
}

// The four face weights of tet k (vertices v) as doubles; need: bit f set =
// face f wanted.  The tet's vertices and metric rows are loaded once and each
// of the six edge lengths is computed once: an edge serves two faces, and
// MMG5_lenedg is a function of (tet, ia), so the values are those of the
// reference's twelve calls.  SURF (tensor metric with surface data or ridge
// storage): len_tet_ani, as k_prilen takes it.
template <bool ANI, bool SURF>
__device__ __forceinline__ void tet_face_weights(const StatArgs &A, int64_t k, const int v[4], unsigned need,
                                                 double w[4]) {
  // edges of face f in MMG5_iarf order; faces that hold edge ia
  constexpr int iarf[4][3] = {{5, 4, 3}, {5, 1, 2}, {4, 2, 0}, {3, 0, 1}};
  constexpr unsigned efaces[6] = {0xcu, 0xau, 0x6u, 0x9u, 0x5u, 0x3u};
  constexpr int e0[6] = {0, 0, 0, 1, 1, 2}, e1[6] = {1, 2, 3, 2, 3, 3};
  double term[6];
  if constexpr (SURF) {
    const unsigned et = A.etag ? (unsigned)A.etag[k] : 0u;
#pragma unroll
    for (int ia = 0; ia < 6; ia++)
      term[ia] = (need & efaces[ia]) ? wgt_term(len_tet_ani(A, v, ia, v[e0[ia]], v[e1[ia]], et)) : 0.0;
  } else if constexpr (ANI) {
    D3 c[4];
    double m[4][6];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      c[j] = sld3(A, v[j]);
      const double *s = smet(A, v[j]);
#pragma unroll
      for (int i = 0; i < 6; i++) m[j][i] = s[i];
    }
#pragma unroll
    for (int ia = 0; ia < 6; ia++)
      term[ia] = (need & efaces[ia]) ? wgt_term(ani_edge_len(c[e0[ia]], c[e1[ia]], m[e0[ia]], m[e1[ia]])) : 0.0;
  } else {
    D3 c[4];
    double h[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      c[j] = sld3(A, v[j]);
      h[j] = smet(A, v[j])[0];
    }
#pragma unroll
    for (int ia = 0; ia < 6; ia++) {
      const IsoEdge e{c[e0[ia]], c[e1[ia]], h[e0[ia]], h[e1[ia]]};
      term[ia] = (need & efaces[ia]) ? wgt_term(iso_edge_len(e)) : 0.0;
    }
  }
#pragma unroll
  for (int f = 0; f < 4; f++) {
    double res = 0.0;
    res += term[iarf[f][0]];
    res += term[iarf[f][1]];
    res += term[iarf[f][2]];
    w[f] = ((need >> f) & 1u) ? wgt_of(res) : PMX_WGT_HUGE;
  }
}

// adjncy (+ adjwgt) of every tet at xadj[k - 1], one thread per tet:
// consecutive threads write consecutive ranges.  The host launches it only
// when xadj[ne] fits the arrays' capacity, so every store is inside them.
// WGT: the weights are wanted; MET: there is a metric (else every weight is
// PMMG_WGTVAL_HUGEINT and no length is computed).
template <bool ANI, bool SURF, bool WGT, bool MET>
__global__ __launch_bounds__(256) void k_graph_fill(StatArgs A, const int *__restrict__ xadj,
                                                    int *__restrict__ adjncy, int *__restrict__ adjwgt) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > A.ne) return;
  const int4 *recs = reinterpret_cast<const int4 *>(A.tets);
  const int4 vv = recs[2 * k], nn = recs[2 * k + 1];
  const int nb[4] = {nn.x, nn.y, nn.z, nn.w};
  unsigned need = 0;
#pragma unroll
  for (int f = 0; f < 4; f++) need |= (nb[f] != 0 ? 1u : 0u) << f;
  if (!need) return;
  int c = xadj[k - 1];
  int iw[4] = {(int)PMX_WGT_HUGE, (int)PMX_WGT_HUGE, (int)PMX_WGT_HUGE, (int)PMX_WGT_HUGE};
  if constexpr (WGT && MET) {
    const int v[4] = {vv.x, vv.y, vv.z, vv.w};
    double w[4];
    tet_face_weights<ANI, SURF>(A, k, v, need, w);
#pragma unroll
    for (int f = 0; f < 4; f++) iw[f] = max((int)w[f], 1);
  }
#pragma unroll
  for (int f = 0; f < 4; f++) {
    if (!nb[f]) continue;
    adjncy[c] = nb[f] - 1;
    if constexpr (WGT) adjwgt[c] = iw[f];
    c++;
  }
}

// PMMG_computeWgt as a double for listed faces: face[i] = 12 ie + 3 ifac (+ iloc)
template <bool ANI, bool SURF, bool MET>
__global__ __launch_bounds__(256) void k_face_weights(StatArgs A, const int *__restrict__ face, int64_t n,
                                                      double *__restrict__ wgt, unsigned *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int fc = face[i];
  const int64_t k = fc / 12;
  const int f = (fc % 12) / 3;
  if (fc < 12 || k > A.ne) { *flag = 1u; return; }
  double out = PMX_WGT_HUGE;
  if constexpr (MET) {
    const int4 vv = reinterpret_cast<const int4 *>(A.tets)[2 * k];
    if (vv.x <= 0) { *flag = 1u; return; }
    const int v[4] = {vv.x, vv.y, vv.z, vv.w};
    double w[4];
    tet_face_weights<ANI, SURF>(A, k, v, 1u << f, w);
    out = f == 0 ? w[0] : f == 1 ? w[1] : f == 2 ? w[2] : w[3];
  }
  wgt[i] = out;
}

// ---- host side ------------------------------------------------------------------

// the lengths' view of the group for PMMG_computeWgt: StatArgs as pmx_prilen
// sets them (ridge storage, surface data); surf = the len_tet_ani variants
static bool graph_args(const pmx_call &C, int metRidTyp, StatArgs &A, bool &surf) {
  if (!stat_args(C, A, false) || !check_met_rid_typ(C, metRidTyp)) return false;
  if (4 * C.ctx->ne >= (1LL << 31)) return C.fail("4 ne >= 2^31 (32-bit idx_t)");
  if (!length_view(C, metRidTyp, A)) return false;
  surf = A.msize == 6 && (C.ctx->have_surf || A.ridmet);
  return true;
}

double pmx_graph_kernel_ms(pmx_ctx *ctx, int which) {
  const int n = ctx->graph_ev_n;
  if (n < 3) return -1.0;
  const pmx_call C{ctx, "pmx_kernel_ms", ctx->stream};
  float cnt = 0.f, scan = 0.f, fill = 0.f;
  if (!C.hip(hipStreamSynchronize(C.s), "graph events") ||
      !C.hip(hipEventElapsedTime(&cnt, ctx->graph_ev[0], ctx->graph_ev[1]), "graph count time") ||
      !C.hip(hipEventElapsedTime(&scan, ctx->graph_ev[1], ctx->graph_ev[2]), "graph scan time") ||
      (n >= 5 && !C.hip(hipEventElapsedTime(&fill, ctx->graph_ev[3], ctx->graph_ev[4]), "graph fill time")))
    return -1.0;
  switch (which) {
    case 9: return cnt;
    case 10: return scan;
    case 11: return fill;
    default: return (double)cnt + scan + fill;
  }
}

extern "C" {

int pmx_metis_graph(pmx_ctx *ctx, int metRidTyp, int32_t *xadj, int32_t *adjncy, int32_t *adjwgt, int64_t cap,
                    int64_t *nadjncy) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_metis_graph", ctx->stream};
  hipSetDevice(ctx->device);
  StatArgs A;
  bool surf = false;
  if (!graph_args(C, metRidTyp, A, surf)) return 0;
  if (!xadj || !nadjncy || cap < 0) return C.fail("xadj / nadjncy are NULL or cap < 0");
  const int64_t ne = ctx->ne;
  hipStream_t s = C.s;
  if (!pmx_create_events(ctx->graph_ev)) return C.fail("event");
  ctx->graph_ev_n = 0;
  size_t tb = 0;
  if (!C.ok(hipcub::DeviceScan::InclusiveSum(nullptr, tb, (const int *)nullptr, (int *)nullptr, (int)(ne + 1), s),
            "scan size"))
    return 0;
  if (!pmx_dgrow(ctx, ctx->d_gdeg, (size_t)(ne + 1)) || !pmx_dgrow(ctx, ctx->d_gxadj, (size_t)(ne + 1)) ||
      !pmx_dgrow(ctx, ctx->d_gflag, 1) || !pmx_dgrow(ctx, ctx->d_gtmp, tb))
    return 0;
  const unsigned nbc = (unsigned)((ne + 1 + 255) / 256), nbf = pmx_call::blocks(ne);
  PMX_CK(C, hipMemsetAsync(ctx->d_gflag.p, 0, sizeof(unsigned), s));
  PMX_CK(C, hipEventRecord(ctx->graph_ev[0], s));
  hipLaunchKernelGGL(k_graph_count, dim3(nbc), dim3(256), 0, s, (const TetRec *)ctx->d_tets.p, ne, ctx->d_gdeg.p,
                     ctx->d_gflag.p);
  PMX_CK(C, hipEventRecord(ctx->graph_ev[1], s));
  if (!C.ok(hipcub::DeviceScan::InclusiveSum(ctx->d_gtmp.p, tb, (const int *)ctx->d_gdeg.p, ctx->d_gxadj.p,
                                             (int)(ne + 1), s),
            "scan"))
    return 0;
  PMX_CK(C, hipEventRecord(ctx->graph_ev[2], s));
  PMX_CK(C, hipGetLastError());
  // the host needs nadjncy (and the flag) before it can size anything
  int tot = 0;
  unsigned flag = 0;
  PMX_CK(C, hipMemcpyAsync(&tot, ctx->d_gxadj.p + ne, sizeof tot, hipMemcpyDeviceToHost, s));
  if (!C.read_words(&flag, (const unsigned *)ctx->d_gflag.p, 1, "count download")) return 0;
  ctx->graph_ev_n = 3;
  if (flag) return C.fail("a deleted tet (v[0] <= 0): the reference wants a packed mesh");
  *nadjncy = tot;
  if (adjncy && tot > cap)
    return C.fail("adjncy holds " + std::to_string(cap) + " entries, nadjncy = " + std::to_string(tot));
  if (adjncy && tot > 0) {
    if (!pmx_dgrow(ctx, ctx->d_gadj, (size_t)tot) || (adjwgt && !pmx_dgrow(ctx, ctx->d_gwgt, (size_t)tot)))
      return 0;
    using KF = void (*)(StatArgs, const int *, int *, int *);
    KF kern = k_graph_fill<false, false, false, false>;
    if (adjwgt) {
      if (A.msize == 0) kern = k_graph_fill<false, false, true, false>;
      else if (surf) kern = k_graph_fill<true, true, true, true>;
      else if (A.msize == 6) kern = k_graph_fill<true, false, true, true>;
      else kern = k_graph_fill<false, false, true, true>;
    }
    PMX_CK(C, hipEventRecord(ctx->graph_ev[3], s));
    hipLaunchKernelGGL(kern, dim3(nbf), dim3(256), 0, s, A, (const int *)ctx->d_gxadj.p, ctx->d_gadj.p,
                       adjwgt ? ctx->d_gwgt.p : (int *)nullptr);
    PMX_CK(C, hipEventRecord(ctx->graph_ev[4], s));
    PMX_CK(C, hipGetLastError());
  }
  PMX_CK(C, hipMemcpyAsync(xadj, ctx->d_gxadj.p, sizeof(int32_t) * (size_t)(ne + 1), hipMemcpyDeviceToHost, s));
  if (adjncy && tot > 0) {
    PMX_CK(C, hipMemcpyAsync(adjncy, ctx->d_gadj.p, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost, s));
    if (adjwgt)
      PMX_CK(C, hipMemcpyAsync(adjwgt, ctx->d_gwgt.p, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost, s));
  }
  PMX_CK(C, hipStreamSynchronize(s));
  if (adjncy && tot > 0) ctx->graph_ev_n = 5;
  return 1;
}

int pmx_face_weights(pmx_ctx *ctx, int metRidTyp, int64_t n, const int *face, double *wgt) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_face_weights", ctx->stream};
  hipSetDevice(ctx->device);
  StatArgs A;
  bool surf = false;
  if (!graph_args(C, metRidTyp, A, surf)) return 0;
  if (n < 0 || (n > 0 && (!face || !wgt))) return C.fail("bad face list");
  if (n == 0) return 1;
  for (int64_t i = 0; i < n; i++)
    if (face[i] < 12 || face[i] / 12 > ctx->ne)
      return C.fail("face[" + std::to_string(i) + "] = " + std::to_string(face[i]) + " is outside 12 .. 12 ne + 11");
  hipStream_t s = C.s;
  if (!pmx_dgrow(ctx, ctx->d_gface, (size_t)n) || !pmx_dgrow(ctx, ctx->d_gfw, (size_t)n) ||
      !pmx_dgrow(ctx, ctx->d_gflag, 1))
    return 0;
  PMX_CK(C, hipMemsetAsync(ctx->d_gflag.p, 0, sizeof(unsigned), s));
  PMX_CK(C, hipMemcpyAsync(ctx->d_gface.p, face, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
  using KW = void (*)(StatArgs, const int *, int64_t, double *, unsigned *);
  KW kern = k_face_weights<false, false, false>;
  if (A.msize != 0) {
    if (surf) kern = k_face_weights<true, true, true>;
    else if (A.msize == 6) kern = k_face_weights<true, false, true>;
    else kern = k_face_weights<false, false, true>;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, (const int *)ctx->d_gface.p, n,
                     ctx->d_gfw.p, ctx->d_gflag.p);
  PMX_CK(C, hipGetLastError());
  unsigned flag = 0;
  if (!C.read_words(&flag, (const unsigned *)ctx->d_gflag.p, 1, "flag download")) return 0;
  if (flag) return C.fail("a listed face belongs to a deleted tet");
  PMX_CK(C, hipMemcpy(wgt, ctx->d_gfw.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return 1;
}

}  // extern "C"
