// pmx_quality.hip -- tet quality and its histogram on gfx950.
//
// pmx_tetra_qual       <- PMMG_tetraQual -> MMG3D_tetraQual (reference
//                         src/quality_pmmg.c:720-733; the per-tet functions
//                         are pmx_metric.h's)
// pmx_qualhisto[_device] <- the per-group part of PMMG_qualhisto
//                         (src/quality_pmmg.c:156-261): MMG3D_computeInqua /
//                         computeOutqua statistics (5 bins, min + location,
//                         max, sum, good, med; OUTQUA: nrid)
// pmx_count_nodes      <- the group's node count (PMMG_count_nodes_par, :33-80)
// pmx_new_mesh_qual[_synced] <- PMMG_tetraQual on the new mesh right after the
//                         interpolation (src/libparmmg1.c:845), in the
//                         device-resident interpolated metric (no re-upload)
//
// k_tet_conn           the statistics' connectivity stream (the tets' vertices,
//                         16 B each) out of the tet records, built on demand
//
// The histogram is one pass over the mesh: per-thread accumulation, a
// wavefront reduction, one partial record per workgroup, and a two-level final
// reduction in workgroup order (deterministic sums).  This file also defines
// the statistics' view of the uploaded group (stat_args) that the edge
// lengths (pmx_lengths.hip) and the Metis graph (pmx_graph.hip) start from.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <vector>
#include "pmx_internal.h"
#include "pmx_metric.h"

#define ALPHAD 20.7846097          // MMG3D_ALPHAD (12*sqrt(3))

// ---- quality histogram ------------------------------------------------------------

struct QualPart {
  double avg, max, min;
  long long iel, ne, good, med, his[5], nrid;
};

__device__ __forceinline__ void qual_merge(QualPart &x, const QualPart &y) {
  x.avg += y.avg;
  x.max = fmax(x.max, y.max);
  if (y.min < x.min || (y.min == x.min && y.iel < x.iel)) { x.min = y.min; x.iel = y.iel; }
  x.ne += y.ne; x.good += y.good; x.med += y.med; x.nrid += y.nrid;
  for (int i = 0; i < 5; i++) x.his[i] += y.his[i];
}
__device__ __forceinline__ void qual_init(QualPart &p) {
  p.avg = 0.0; p.max = 0.0; p.min = 2.0; p.iel = 0x7fffffffffffffffLL;
  p.ne = 0; p.good = 0; p.med = 0; p.nrid = 0;
  for (int i = 0; i < 5; i++) p.his[i] = 0;
}

// quality of every tet (+ optional histogram partials in the same pass).
// ANI: the metric is a 6-component tensor (compiled apart: the iso variant
// does not carry the tensor path's registers).  OUT: MMG3D_computeOutqua's
// count of tets with 4 ridge vertices.
// Each workgroup takes a contiguous tet range, 256 tets per iteration, the
// next iteration's connectivity loaded before this one's vertex gathers (two
// dependent levels in flight).  Counts are wave-uniform (ballot + popcount,
// scalar registers); sum and extrema per lane, reduced by a fixed shuffle
// tree and the 4 waves in order (deterministic), so the workgroup needs no
// 256-entry LDS reduction buffer (occupancy no longer LDS-bound).
// MODE (compiled apart, no run-time branches in the loop): QM_STORE every
// tet's quality into qual, no partials (MMG3D_tetraQual); QM_HISTO the
// partials of freshly computed qualities, nothing stored; QM_STORED the
// partials of the qualities already in qual (OUTQUA after tetraQual).
enum { QM_STORE = 0, QM_HISTO = 1, QM_STORED = 2 };
template <bool ANI, bool OUT, int MODE>
__global__ __launch_bounds__(256) void k_qual(StatArgs A, double *qual, QualPart *parts) {
  constexpr bool use_stored = MODE == QM_STORED;
  __shared__ QualPart sh[4];
  double avg = 0.0, qmax = 0.0, qmin = 2.0;
  long long iel = 0x7fffffffffffffffLL;
  unsigned cne = 0, cgood = 0, cmed = 0, cnrid = 0, chis[5] = {0, 0, 0, 0, 0};
  // contiguous chunk per block; each XCD gets a contiguous run of chunks so
  // the next z-layer's points (another chunk) are in its own L2
  const int64_t lb = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t per = (A.ne + gridDim.x - 1) / gridDim.x;
  const int64_t k0 = 1 + lb * per, k1 = min(A.ne, k0 + per - 1), kstep = blockDim.x;
  // 16-B connectivity stream: the neighbours are not needed here
  int4 cv = (k0 + (int64_t)threadIdx.x <= k1) ? A.tetv[k0 + threadIdx.x] : make_int4(0, 0, 0, 0);
  // the vertex rows are loaded for every lane (an invalid tet reads row 0 and
  // discards the result), then the next connectivity: loads return in
  // order, so a prefetch issued before the gathers (r05) made every gather
  // wait for it -- the prefetch hid nothing.  The ridge-storage mean
  // (OUTQUA with a tensor metric) keeps the tag-dependent loads.
  const bool pre = !(ANI && A.ridmet);
  for (int64_t kb = k0; kb <= k1; kb += kstep) {   // uniform over the block
    const int64_t k = kb + threadIdx.x;
    const bool in = k <= k1;
    const int v[4] = {cv.x, cv.y, cv.z, cv.w};
    const bool valid = in && v[0] > 0;
    const int64_t kn = k + kstep;
    double q = 0.0;
    bool rid4 = false;
    if (use_stored || pre) {
      const int vb = A.vbase;
      const int w[4] = {valid ? v[0] : vb, valid ? v[1] : vb, valid ? v[2] : vb, valid ? v[3] : vb};
      unsigned tg[4] = {0u, 0u, 0u, 0u};
      if (OUT && A.ptag) {
#pragma unroll
        for (int i = 0; i < 4; i++) tg[i] = stag(A, w[i]);
      }
      double qs = 0.0;
      D3 P[4];
      double mv[ANI ? 4 : 1][6];
      if constexpr (use_stored) {
        qs = qual[in ? k : k1];
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) P[i] = sld3(A, w[i]);
        if constexpr (ANI) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const double *m = smet(A, w[i]);
#pragma unroll
            for (int j = 0; j < 6; j++) mv[i][j] = m[j];
          }
        }
      }
      cv = A.tetv[kn <= k1 ? kn : k1];
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (use_stored) {
        q = qs;
      } else if constexpr (ANI) {
        q = caltet_ani(P[0], P[1], P[2], P[3], mv[0], mv[1], mv[2], mv[3]);
      } else {
        q = caltet_iso(P[0], P[1], P[2], P[3]);
      }
      if (OUT && A.ptag) rid4 = ridge_pt(tg[0]) && ridge_pt(tg[1]) && ridge_pt(tg[2]) && ridge_pt(tg[3]);
    } else {
      if (kn <= k1) cv = A.tetv[kn];
      if (valid) q = tet_quality<ANI>(A, v);
      if (OUT && valid) rid4 = tet_4ridge(A, v);
    }
    // !MG_EOK: no quality (0, not a stale value)
    if (MODE == QM_STORE && in && !valid) qual[k] = 0.0;
    double rap = 0.0;
    if (valid) {
      if (MODE == QM_STORE) qual[k] = q;
      rap = ALPHAD * q;
      if (MODE != QM_STORE) {
        if (rap < qmin || (rap == qmin && k < iel)) { qmin = rap; iel = k; }
        avg += rap;
        qmax = fmax(qmax, rap);
      }
    }
    if (MODE == QM_STORE) continue;
    cne += (unsigned)__popcll(__ballot(valid));
    cgood += (unsigned)__popcll(__ballot(valid && rap > 0.12));
    cmed += (unsigned)__popcll(__ballot(valid && rap > 0.5));
    if (OUT) cnrid += (unsigned)__popcll(__ballot(valid && rid4));
    int ir = (int)(5.0 * rap);
    ir = ir < 4 ? ir : 4;
    // the bin from three bit ballots (scalar mask algebra) instead of five
    // per-bin ones
    const unsigned long long V = __ballot(valid), B0 = __ballot(ir & 1), B1 = __ballot(ir & 2),
                             B2 = __ballot(ir & 4);
    const unsigned long long L = V & ~B2;            // bins 0-3
    chis[0] += (unsigned)__popcll(L & ~B1 & ~B0);
    chis[1] += (unsigned)__popcll(L & ~B1 & B0);
    chis[2] += (unsigned)__popcll(L & B1 & ~B0);
    chis[3] += (unsigned)__popcll(L & B1 & B0);
    chis[4] += (unsigned)__popcll(V & B2);
  }
  if (MODE == QM_STORE) return;
  // the same tree on every lane (the lower lane's value first)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double ya = __shfl_xor(avg, o, 64), ymx = __shfl_xor(qmax, o, 64), ymn = __shfl_xor(qmin, o, 64);
    const long long yi = __shfl_xor(iel, o, 64);
    avg = (threadIdx.x & o) == 0 ? avg + ya : ya + avg;
    qmax = fmax(qmax, ymx);
    if (ymn < qmin || (ymn == qmin && yi < iel)) { qmin = ymn; iel = yi; }
  }
  if ((threadIdx.x & 63) == 0) {
    QualPart p;
    p.avg = avg; p.max = qmax; p.min = qmin; p.iel = iel;
    p.ne = cne; p.good = cgood; p.med = cmed; p.nrid = cnrid;
#pragma unroll
    for (int i = 0; i < 5; i++) p.his[i] = chis[i];
    sh[threadIdx.x >> 6] = p;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    QualPart r = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) qual_merge(r, sh[w]);
    parts[lb] = r;
  }
}

// fixed-order reduction of n partials (launched twice: FINAL_GRID blocks, then
// one); the last level writes the public pmx_qual_part (np from the node count)
__global__ __launch_bounds__(256) void k_qual_final(const QualPart *parts, int n, QualPart *res,
                                                    pmx_qual_part *pub, long long np) {
  __shared__ QualPart sh[256];
  QualPart p;
  qual_init(p);
  const int pb = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * pb, hi = min(n, lo + pb);
  int per = (hi - lo + 255) / 256;
  for (int b = lo + threadIdx.x * per; b < min(hi, lo + (int)(threadIdx.x + 1) * per); b++)
    qual_merge(p, parts[b]);
  sh[threadIdx.x] = p;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) qual_merge(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (res) res[blockIdx.x] = sh[0];
  if (pub) {
    const QualPart &r = sh[0];
    pmx_qual_part o;
    o.avg = r.avg; o.max = r.max; o.min = r.min;
    o.iel = r.ne ? r.iel : 0;
    o.ne = r.ne; o.np = np; o.good = r.good; o.med = r.med; o.nrid = r.nrid;
    for (int i = 0; i < 5; i++) o.his[i] = r.his[i];
    o.iel_grp = 0;
    *pub = o;
  }
}

// ---- node count (PMMG_count_nodes_par, src/quality_pmmg.c:33-80) ------------------

// points touched by a valid tet
__global__ __launch_bounds__(256) void k_touch(const int4 *__restrict__ tv, int64_t ne,
                                               uint8_t *__restrict__ touched) {
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= ne;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int4 v = tv[k];
    if (v.x <= 0) continue;
    touched[v.x] = 1; touched[v.y] = 1; touched[v.z] = 1; touched[v.w] = 1;
  }
}
// points of the internal node communicator count when they claim their slot
// (intvalues[idx] == 0 -> base); the other points when a valid tet touches them
__global__ __launch_bounds__(256) void k_count_nodes(const uint8_t *__restrict__ touched, int64_t np,
                                                     const int *__restrict__ comm_idx,
                                                     int *__restrict__ intvalues, int base,
                                                     unsigned long long *__restrict__ count) {
  unsigned c = 0;
  for (int64_t ip = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ip <= np;
       ip += (int64_t)gridDim.x * blockDim.x) {
    const int idx = comm_idx ? comm_idx[ip] : -1;
    if (idx >= 0) c += atomicCAS(&intvalues[idx], 0, base) == 0 ? 1u : 0u;
    else c += touched[ip] ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// ---- host side ------------------------------------------------------------------

// partial records per pass: a function of ne only (the fixed-order final
// reduction then gives the same sums on every run); enough workgroups to fill
// 256 CUs several times over, each a contiguous range of >= 2048 tets
int stat_blocks(int64_t ne) {
  return (int)std::max<int64_t>(256, std::min<int64_t>(16384, ne / 2048));
}

// connectivity stream out of the tet records (statistics pass, built on demand)
__global__ __launch_bounds__(256) void k_tet_conn(const TetRec *__restrict__ src, int64_t n,
                                                  int4 *__restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = *reinterpret_cast<const int4 *>(src + i);
}
static void launch_tet_conn(const TetRec *src, int64_t n, int4 *dst, hipStream_t s) {
  hipLaunchKernelGGL(k_tet_conn, dim3(pmx_grid(n, 16384)), dim3(256), 0, s, src, n, dst);
}

bool ensure_tetv(pmx_ctx *ctx) {
  if (ctx->have_tetv) return true;
  if (!pmx_dgrow(ctx, ctx->d_tetv, (size_t)(ctx->ne + 1))) return false;
  launch_tet_conn(ctx->d_tets.p, ctx->ne + 1, ctx->d_tetv.p, ctx->stream);
  ctx->have_tetv = true;
  return true;
}

// the statistics' view of the background group
bool stat_args(const pmx_call &C, StatArgs &A, bool tetv) {
  pmx_ctx *ctx = C.ctx;
  if (!ctx->have_bg) return C.fail("upload a group first");
  // the 16-B connectivity stream of the quality pass, derived from the tet
  // records on the first statistics call after an upload (the transfer step
  // itself does not need it; nor does the Metis graph: tetv false)
  if (tetv && !ensure_tetv(ctx)) return false;
  A = StatArgs{};
  A.xyz = ctx->d_xyz.p;
  A.xstride = 3;
  A.vbase = 0;
  A.tets = ctx->d_tets.p;
  A.tetv = ctx->d_tetv.p;
  A.ne = ctx->ne;
  A.sol = ctx->d_sol.p;
  A.S = ctx->sd.S;
  A.msize = ctx->sd.imet >= 0 ? ctx->sd.size[ctx->sd.imet] : 0;
  A.moff = ctx->sd.imet >= 0 ? ctx->sd.off[ctx->sd.imet] : 0;
  A.ptag = ctx->have_ptag ? ctx->d_ptag.p : nullptr;
  return true;
}

bool ensure_red(pmx_ctx *ctx, size_t bytes) {
  return pmx_dgrow(ctx, ctx->d_red, (bytes + 7) / 8);
}

// metRidTyp selects Mmg's ridge-metric storage (src/quality_pmmg.c:462,527,
// 726).  For a size-1 metric (or none) both values take the same isotropic
// arithmetic.  With a size-6 metric:
//  * the quality (MMG3D_tetraQual: 0 -> MMG5_caltet33_ani, 1 -> MMG5_orcal ->
//    MMG5_caltet_ani) is restated for both: 1 averages the metric over the
//    vertices that are not non-singular ridge points (MMG5_moymet), which
//    needs the point tags (caltet_ani_rid);
//  * the edge lengths (0: MMG5_lenedg33_ani, 1: MMG5_lenedg_ani) measure the
//    xTetra's boundary edges along the curved surface (pmx_upload_surface),
//    and 1 rebuilds a ridge point's metric per direction (MMG5_buildridmet)
//    or takes the tet's mean (MMG5_lenedgspl_ani): len_tet_ani.
bool check_met_rid_typ(const pmx_call &C, int metRidTyp) {
  return metRidTyp == 0 || metRidTyp == 1 || C.fail("metRidTyp must be 0 or 1");
}

// MMG3D_tetraQual: the quality of every tet of the mesh described by A into
// qual (device), the kernel by metric size
static void launch_qual_store(const StatArgs &A, double *qual, hipStream_t s) {
  const dim3 grid(stat_blocks(A.ne)), block(256);
  if (A.msize == 6)
    hipLaunchKernelGGL((k_qual<true, false, QM_STORE>), grid, block, 0, s, A, qual, (QualPart *)nullptr);
  else
    hipLaunchKernelGGL((k_qual<false, false, QM_STORE>), grid, block, 0, s, A, qual, (QualPart *)nullptr);
}

// qualhisto partial of the mesh described by A (background or new mesh)
static bool qual_partial(const pmx_call &C, const StatArgs &A, int opt, double *qual_dev, int use_stored,
                         pmx_qual_part *pub, long long np) {
  const int nb = stat_blocks(A.ne);
  if (!ensure_red(C.ctx, sizeof(QualPart) * (nb + FINAL_GRID + 1))) return false;
  QualPart *parts = (QualPart *)C.ctx->d_red.p;
  const bool ani = A.msize == 6, out = opt == PMX_OUTQUA && A.ptag;
  double *q = use_stored ? qual_dev : nullptr;
  // MMG3D_computeInqua takes MMG5_caltet33_ani (classic storage);
  // MMG3D_computeOutqua MMG5_orcal -> MMG5_caltet_ani, the ridge-storage mean
  // (ridge points left out, caltet_ani_rid) -- unless the caller's stored
  // qualities are used
  StatArgs B = A;
  if (ani && opt == PMX_OUTQUA && !use_stored) {
    B.ridmet = 1;
    B.rtag = A.ptag;
  }
  using KQ = void (*)(StatArgs, double *, QualPart *);
  static const KQ kq[2][2][2] = {
      {{k_qual<false, false, QM_HISTO>, k_qual<false, false, QM_STORED>},
       {k_qual<false, true, QM_HISTO>, k_qual<false, true, QM_STORED>}},
      {{k_qual<true, false, QM_HISTO>, k_qual<true, false, QM_STORED>},
       {k_qual<true, true, QM_HISTO>, k_qual<true, true, QM_STORED>}}};
  hipLaunchKernelGGL(kq[ani][out][use_stored ? 1 : 0], dim3(nb), dim3(256), 0, C.s, B, q, parts);
  QualPart *mid = parts + nb;
  hipLaunchKernelGGL(k_qual_final, dim3(FINAL_GRID), dim3(256), 0, C.s, parts, nb, mid,
                     (pmx_qual_part *)nullptr, 0LL);
  hipLaunchKernelGGL(k_qual_final, dim3(1), dim3(256), 0, C.s, mid, FINAL_GRID, (QualPart *)nullptr, pub, np);
  return C.hip(hipGetLastError(), "histogram launch");
}

extern "C" {

int pmx_upload_point_tags(pmx_ctx *ctx, const uint16_t *tag, int64_t stride) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_upload_point_tags", ctx->stream};
  ctx->have_ptag = false;
  if (!ctx->have_bg) return C.fail("upload a background first");
  if (!tag) return 1;                       // no tags: no ridge points
  hipSetDevice(ctx->device);
  const int64_t np = ctx->np;
  char *st = pmx_hstage(ctx, (size_t)(np + 1) * 2);
  if (!st) return 0;
  uint16_t *h = (uint16_t *)st;
  h[0] = 0;
  for (int64_t i = 1; i <= np; i++) h[i] = *(const uint16_t *)((const char *)tag + i * stride);
  if (!pmx_dgrow(ctx, ctx->d_ptag, (size_t)(np + 1))) return 0;
  PMX_CK(C, hipMemcpyAsync(ctx->d_ptag.p, h, (size_t)(np + 1) * 2, hipMemcpyHostToDevice, C.s));
  PMX_CK(C, hipStreamSynchronize(C.s));
  ctx->have_ptag = true;
  return 1;
}

int pmx_tetra_qual(pmx_ctx *ctx, int metRidTyp, double *qual, int64_t qual_cap) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_tetra_qual", ctx->stream};
  hipSetDevice(ctx->device);
  StatArgs A;
  if (!stat_args(C, A) || !check_met_rid_typ(C, metRidTyp)) return 0;
  if (qual && qual_cap < ctx->ne + 1)
    return C.fail("qual holds " + std::to_string(qual_cap) + " doubles, ne+1 = " + std::to_string(ctx->ne + 1) +
                  " needed");
  A.ridmet = metRidTyp == 1 && A.msize == 6;
  A.rtag = A.ptag;
  if (A.ridmet && !A.rtag)
    return C.fail("metRidTyp = 1 with a tensor metric needs the point tags (pmx_upload_point_tags)");
  if (!pmx_dgrow(ctx, ctx->d_qual, (size_t)(ctx->ne + 1))) return 0;
  launch_qual_store(A, ctx->d_qual.p, C.s);
  PMX_CK(C, hipGetLastError());
  ctx->have_qual = true;
  if (qual) {
    PMX_CK(C, hipStreamSynchronize(C.s));
    PMX_CK(C, hipMemcpy(qual, ctx->d_qual.p, sizeof(double) * (size_t)(ctx->ne + 1), hipMemcpyDeviceToHost));
    qual[0] = 0.0;
  }
  return 1;
}

int pmx_count_nodes(pmx_ctx *ctx, const int *idx_ip, const int *idx_comm, int64_t nitem_grp,
                    int *intvalues, int64_t nitem, int base, int64_t *np_out) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_count_nodes", ctx->stream};
  if (!np_out) return C.fail("np_out is NULL");
  hipSetDevice(ctx->device);
  StatArgs A;
  if (!stat_args(C, A)) return 0;
  if (nitem_grp < 0 || nitem < 0 || (nitem_grp > 0 && (!idx_ip || !idx_comm || !intvalues)))
    return C.fail("bad communicator arrays");
  const int64_t np = ctx->np;
  hipStream_t s = C.s;
  // point -> communicator slot (-1: not in the internal communicator)
  std::vector<int> cidx;
  if (nitem_grp > 0) {
    cidx.assign((size_t)(np + 1), -1);
    for (int64_t i = 0; i < nitem_grp; i++) {
      if (idx_ip[i] < 1 || idx_ip[i] > np || idx_comm[i] < 0 || idx_comm[i] >= nitem)
        return C.fail("communicator index out of range");
      cidx[(size_t)idx_ip[i]] = idx_comm[i];
    }
  }
  if (!pmx_dgrow(ctx, ctx->d_touch, (size_t)(np + 1)) || !pmx_dgrow(ctx, ctx->d_cidx, cidx.size() + 1) ||
      !pmx_dgrow(ctx, ctx->d_intv, (size_t)std::max<int64_t>(nitem, 1)) || !ensure_red(ctx, 64))
    return 0;
  unsigned long long *cnt = ctx->d_red.p;
  PMX_CK(C, hipMemsetAsync(ctx->d_touch.p, 0, (size_t)(np + 1), s));
  PMX_CK(C, hipMemsetAsync(cnt, 0, 8, s));
  if (nitem_grp > 0) {
    PMX_CK(C, hipMemcpyAsync(ctx->d_cidx.p, cidx.data(), cidx.size() * 4, hipMemcpyHostToDevice, s));
    PMX_CK(C, hipMemcpyAsync(ctx->d_intv.p, intvalues, (size_t)nitem * 4, hipMemcpyHostToDevice, s));
  }
  const int64_t nbt = std::min<int64_t>((ctx->ne + 255) / 256, 16384);
  hipLaunchKernelGGL(k_touch, dim3((unsigned)std::max<int64_t>(nbt, 1)), dim3(256), 0, s, A.tetv, ctx->ne,
                     ctx->d_touch.p);
  const int64_t nbp = std::min<int64_t>((np + 255) / 256, 16384);
  hipLaunchKernelGGL(k_count_nodes, dim3((unsigned)std::max<int64_t>(nbp, 1)), dim3(256), 0, s,
                     ctx->d_touch.p, np, nitem_grp > 0 ? ctx->d_cidx.p : nullptr, ctx->d_intv.p, base, cnt);
  if (nitem_grp > 0)
    PMX_CK(C, hipMemcpyAsync(intvalues, ctx->d_intv.p, (size_t)nitem * 4, hipMemcpyDeviceToHost, s));
  unsigned long long c = 0;
  if (!C.read_words(&c, (const unsigned long long *)cnt, 1, "node count")) return 0;
  *np_out = (int64_t)c;
  ctx->stat_np = (int64_t)c;
  return 1;
}

int pmx_qualhisto_device(pmx_ctx *ctx, int opt, int use_stored, void *dev_result) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_qualhisto", ctx->stream};
  if (!dev_result) return C.fail("dev_result is NULL");
  // MMG3D_computeLESqua (src/quality_pmmg.c:221-224, selected at run time by
  // mesh->info.optimLES): Mmg's LES quality is not restated here
  if (opt == PMX_LESQUA) return C.fail("the optimLES quality (MMG3D_computeLESqua) is not supported");
  if (opt != PMX_INQUA && opt != PMX_OUTQUA) return C.fail("opt must be PMX_INQUA, PMX_OUTQUA or PMX_LESQUA");
  hipSetDevice(ctx->device);
  StatArgs A;
  if (!stat_args(C, A)) return 0;
  if (use_stored && !ctx->have_qual) return C.fail("no stored quality");
  const long long np = ctx->stat_np >= 0 ? ctx->stat_np : ctx->np;
  return qual_partial(C, A, opt, ctx->d_qual.p, use_stored, (pmx_qual_part *)dev_result, np);
}

int pmx_qualhisto(pmx_ctx *ctx, int opt, pmx_qual_stats *st) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_qualhisto", ctx->stream};
  if (!st) return C.fail("st is NULL");
  hipSetDevice(ctx->device);
  if (!pmx_dgrow(ctx, ctx->d_pub, 32)) return 0;
  if (!pmx_qualhisto_device(ctx, opt, 0, ctx->d_pub.p)) return 0;
  pmx_qual_part r;
  if (!read_pub(C, r)) return 0;
  qual_to_stats(r, st);
  return 1;
}

// the quality pass over the device-resident new mesh (the step's points and
// the uploaded new tets), in the metric at sol[S * j + moff] (msize 0: none)
static int new_mesh_qual_core(const pmx_call &C, int opt, int metRidTyp, double *qual, int64_t qstride,
                              void *dev_result, const double *sol, int S, int msize, int moff) {
  pmx_ctx *ctx = C.ctx;
  const int64_t ne = ctx->ntets.n;
  const int64_t n = ctx->nq;
  if (!pmx_dgrow(ctx, ctx->d_nqual, (size_t)(ne + 1))) return 0;
  StatArgs A{};
  A.xyz = ctx->d_qxyz.p;                  // the new points, dense x y z
  A.xstride = 3;
  A.vbase = 1;
  A.tetv = ctx->ntets.d_v.p;
  A.ne = ne;
  A.sol = sol;
  A.S = S;
  A.msize = msize;
  A.moff = moff;
  A.ptag = (opt == PMX_OUTQUA && ctx->have_qtag) ? ctx->d_qtag.p : nullptr;
  if (!check_met_rid_typ(C, metRidTyp)) return 0;
  A.ridmet = metRidTyp == 1 && A.msize == 6;
  A.rtag = ctx->have_qtag ? ctx->d_qtag.p : nullptr;
  // MMG5_moymet leaves the ridge points out: without their tags the mean
  // would silently be the plain one
  if (A.ridmet && !A.rtag)
    return C.fail("metRidTyp = 1 with a tensor metric needs the new points' tags (points view tag)");
  if (dev_result && opt != PMX_INQUA && opt != PMX_OUTQUA)
    return C.fail(opt == PMX_LESQUA ? "the optimLES quality (MMG3D_computeLESqua) is not supported"
                                    : "opt must be PMX_INQUA or PMX_OUTQUA");
  launch_qual_store(A, ctx->d_nqual.p, C.s);
  if (dev_result && !qual_partial(C, A, opt, ctx->d_nqual.p, 1, (pmx_qual_part *)dev_result, n)) return 0;
  PMX_CK(C, hipGetLastError());
  if (qual && !pmx_download_qual(ctx, ctx->d_nqual.p, ne, qual, qstride)) return C.fail(ctx->err);
  return 1;
}

int pmx_new_mesh_qual(pmx_ctx *ctx, const int *tetra_v, int64_t tetra_stride, int64_t ne, int opt,
                      int metRidTyp, double *qual, int64_t qual_cap, void *dev_result) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_new_mesh_qual", ctx->stream};
  hipSetDevice(ctx->device);
  if (!ctx->stepped()) return C.fail("run a step on the new points first");
  // the new tets: given here (uploaded, as pmx_upload_new_tets), or NULL for
  // the ones already uploaded; vertex j+1 = new point j
  if (tetra_v) {
    if (!pmx_upload_new_tets(ctx, tetra_v, tetra_stride, ne)) return 0;
  } else if (!ctx->ntets.have) {
    return C.fail("no new tets uploaded");
  } else if (!ctx->ntets.ensure_tets(C.s)) {
    return 0;
  }
  if (qual && qual_cap < ctx->ntets.n + 1)
    return C.fail("qual holds " + std::to_string(qual_cap) + " doubles, ne+1 = " + std::to_string(ctx->ntets.n + 1) +
                  " needed");
  // the interpolated metric, in the step's output rows (a constant-size
  // metric of the step is there too)
  const int msize = ctx->sd.imet >= 0 ? ctx->sd.size[ctx->sd.imet] : 0;
  const int moff = ctx->sd.imet >= 0 ? ctx->sd.off[ctx->sd.imet] : 0;
  return new_mesh_qual_core(C, opt, metRidTyp, qual, 8, dev_result, ctx->d_out.p, ctx->sd.S, msize, moff);
}

// PMMG_tetraQual after PMMG_interpMetricsAndFields on the caller's metric
// array: the step's own rows where it wrote the metric, and only the rows it
// did not write (frozen points that PMMG_copyMetricsAndFields_point filled on
// the host, failed tensor inversions) sent to the device; a metric the step
// did not interpolate (-hsiz constant size, or Mmg's own) is sent whole.
int pmx_new_mesh_qual_synced(pmx_ctx *ctx, const pmx_sol_view *met, int opt, int metRidTyp, double *qual,
                             int64_t qual_stride, int64_t qual_cap, void *dev_result) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_new_mesh_qual_synced", ctx->stream};
  hipSetDevice(ctx->device);
  const int64_t qs = qual_stride ? qual_stride : (int64_t)sizeof(double);
  if (qs < (int64_t)sizeof(double)) return C.fail("bad quality stride");
  if (!ctx->stepped()) return C.fail("run a step on the new points first");
  if (!ctx->ntets.have) return C.fail("the step's points view had no new tets");
  if (qual && qual_cap < ctx->ntets.n + 1)
    return C.fail("qual holds " + std::to_string(qual_cap) + " records, ne+1 = " + std::to_string(ctx->ntets.n + 1) +
                  " needed");
  if (!ctx->ntets.ensure_tets(C.s) || !ctx->ntets.fix_orphans()) return 0;
  const int64_t n = ctx->nq, first = ctx->pts_first;
  hipStream_t s = C.s;
  if (!met || !met->m) return new_mesh_qual_core(C, opt, metRidTyp, qual, qs, dev_result, nullptr, 0, 0, 0);
  const int sz = met->size;
  if (sz != 1 && sz != 6) return C.fail("metric size must be 1 or 6");
  const double *hm = met->m + first * sz;      // Mmg layout: entry of point `first`
  const int im = ctx->sd.imet;
  if (im >= 0 && ctx->sd.size[im] == sz) {
    // the step's metric: patch the rows it did not write from the caller's array
    std::vector<uint8_t> wm((size_t)std::max<int64_t>(n, 1));
    if (n && !C.read_words(wm.data(), (const uint8_t *)ctx->d_wmask.p, (size_t)n, "write masks")) return 0;
    // the unwritten rows, found by the host pool (per-chunk lists joined in order)
    std::vector<int4> ent;
    std::vector<double> val;
    {
      std::mutex mu;
      std::vector<std::pair<int64_t, std::vector<int>>> rows;
      pmx_par_for(0, n, [&](int64_t j0, int64_t j1) {
        std::vector<int> r;
        for (int64_t j = j0; j < j1; j++)
          if (!(wm[(size_t)j] & (1u << im))) r.push_back((int)j);
        std::lock_guard<std::mutex> g(mu);
        rows.emplace_back(j0, std::move(r));
      });
      std::sort(rows.begin(), rows.end(),
                [](const std::pair<int64_t, std::vector<int>> &a, const std::pair<int64_t, std::vector<int>> &b) {
                  return a.first < b.first;
                });
      for (const auto &r : rows)
        for (int j : r.second) {
          ent.push_back(make_int4(j, ctx->sd.off[im], sz, 0));
          for (int c = 0; c < 6; c++) val.push_back(c < sz ? hm[(int64_t)j * sz + c] : 0.0);
        }
    }
    const int64_t ne_ = (int64_t)ent.size();
    if (ne_) {
      if (!pmx_dgrow(ctx, ctx->d_pent, (size_t)ne_) || !pmx_dgrow(ctx, ctx->d_pval, (size_t)ne_ * 6)) return 0;
      PMX_CK(C, hipMemcpyAsync(ctx->d_pent.p, ent.data(), (size_t)ne_ * sizeof(int4), hipMemcpyHostToDevice, s));
      PMX_CK(C, hipMemcpyAsync(ctx->d_pval.p, val.data(), (size_t)ne_ * 6 * sizeof(double), hipMemcpyHostToDevice, s));
      launch_patch_rows(ctx->d_pent.p, ctx->d_pval.p, ne_, ctx->sd.S, ctx->d_out.p, s);
      ctx->eager_nch = 0;                    // the results changed
      // the rows are the caller's now (pmx_download / pmx_promote_background
      // then give the same values)
      const uint8_t bit = (uint8_t)(1u << im);
      for (int64_t e = 0; e < ne_; e++) wm[(size_t)ent[(size_t)e].x] |= bit;
      PMX_CK(C, hipMemcpyAsync(ctx->d_wmask.p, wm.data(), (size_t)n, hipMemcpyHostToDevice, s));
      PMX_CK(C, hipStreamSynchronize(s));
    }
    return new_mesh_qual_core(C, opt, metRidTyp, qual, qs, dev_result, ctx->d_out.p, ctx->sd.S, sz, ctx->sd.off[im]);
  }
  // no metric in the step: the caller's whole array
  if (!pmx_dgrow(ctx, ctx->d_cmet, (size_t)std::max<int64_t>(n * sz, 1))) return 0;
  if (n) {
    PMX_CK(C, hipMemcpyAsync(ctx->d_cmet.p, hm, (size_t)(n * sz) * sizeof(double), hipMemcpyHostToDevice, s));
    PMX_CK(C, hipStreamSynchronize(s));
  }
  return new_mesh_qual_core(C, opt, metRidTyp, qual, qs, dev_result, ctx->d_cmet.p, sz, sz, 0);
}

}  // extern "C"
