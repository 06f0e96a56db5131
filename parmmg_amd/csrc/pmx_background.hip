// pmx_background.hip -- how a mesh becomes the uploaded group, host side and
// kernels.
//
// k_build_tetrec     tet records (+ the every-4th-tet hint sample) from the
//                    connectivity and its Mmg face adjacency
// k_build_wrec       the walk's compact records from the tet records
// k_promote,         a promotion: the step's points and results as vertex and
// k_patch_rows       solution rows; the rows the step did not write
// k_gather_rows      an adopted split group's rows, gathered by index
// k_tri_records      Mmg-layout trias and adjt on the device -> tria records
//
// Three entry points install a background: pmx_upload_background (from the
// host's Mmg arrays), pmx_promote_background (the last step's points and
// results, already on the device) and pmx_ctx_adopt_group (a merged group, or
// one group of another context's split plan, on the device).  Each is
// begin_background, grow_background, its own transfers, build_records,
// finish_background.  build_records is the one place where connectivity
// becomes tet records, and the only code that touches d_adja.
// pmx_download_surface reads the installed trias back.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>

#include "pmx_transfer.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"

// ---- the kernels: records and rows of a background ---------------------------------

// tet records from the new tets and their Mmg face adjacency
// (adja[4*(k-1)+1+f] = 4*k'+f'), and the packed hint sample
__global__ __launch_bounds__(256) void k_build_tetrec(const int4 *__restrict__ tv, const int *__restrict__ adja,
                                                      int64_t ne, int stride, TetRec *__restrict__ tets,
                                                      int4 *__restrict__ sample) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= ne;
       k += (int64_t)gridDim.x * blockDim.x) {
    TetRec r;
    const int4 v = tv[k];
    r.v[0] = v.x; r.v[1] = v.y; r.v[2] = v.z; r.v[3] = v.w;
    for (int f = 0; f < 4; f++) r.nb[f] = k ? adja[4 * (k - 1) + 1 + f] / 4 : 0;
    tets[k] = r;
    if (k >= 1 && (k - 1) % stride == 0) sample[(k - 1) / stride] = v;
  }
}
static void launch_build_tetrec(const int4 *tv, const int *adja, int64_t ne, int stride, TetRec *tets, int4 *sample,
                                hipStream_t s) {
  hipLaunchKernelGGL(k_build_tetrec, dim3(pmx_grid(ne + 1, 16384)), dim3(256), 0, s, tv, adja, ne, stride, tets,
                     sample);
}

// the walk's compact records (WRec, pmx_device.h) from the tet records, built
// with them at every upload / promotion (a re-layout of the connectivity, like
// the records themselves)
__global__ __launch_bounds__(256) void k_build_wrec(const TetRec *__restrict__ tets, int64_t ne,
                                                    WRec *__restrict__ wr, unsigned *__restrict__ nfar) {
  unsigned cnt = 0;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= ne;
       k += (int64_t)gridDim.x * blockDim.x) {
    WRec r;
    wrec_encode(tets[k], k, r);
    wr[k] = r;
    const TetRec d = wrec_decode(r, tets, (int)k);
    cnt += (d.nb[0] | d.nb[1] | d.nb[2] | d.nb[3]) < 0 ? 1u : 0u;
  }
  // tets with a far neighbour field, one atomic per wave
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(nfar, cnt);
}
// slots 0..ne; *h_nfar (pinned), when stream s gets there: the tets with a far
// neighbour field (pmx_wrec.h); d_nfar one device word
static void launch_build_wrec(const TetRec *tets, int64_t ne, WRec *wr, unsigned *d_nfar, unsigned *h_nfar,
                              hipStream_t s) {
  hipMemsetAsync(d_nfar, 0, sizeof(unsigned), s);
  hipLaunchKernelGGL(k_build_wrec, dim3(pmx_grid(ne + 1, 16384)), dim3(256), 0, s, tets, ne, wr, d_nfar);
  hipMemcpyAsync(h_nfar, d_nfar, sizeof(unsigned), hipMemcpyDeviceToHost, s);
}

// device residency across iterations (pmx_promote_background): the last
// step's new points and results become the background: vertex ip (1..n) = new
// point ip-1, its solution row = the step's output row ip-1
__global__ __launch_bounds__(256) void k_promote(const double *__restrict__ q, const double *__restrict__ out,
                                                 const uint16_t *__restrict__ qtag, int64_t n, int S,
                                                 double *__restrict__ xyz, double *__restrict__ sol,
                                                 uint16_t *__restrict__ ptag) {
  for (int64_t ip = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ip <= n;
       ip += (int64_t)gridDim.x * blockDim.x) {
    if (ip == 0) {
      xyz[0] = xyz[1] = xyz[2] = 0.0;
      for (int j = 0; j < S; j++) sol[j] = 0.0;
      if (ptag) ptag[0] = 0;
      continue;
    }
    xyz[3 * ip] = q[3 * (ip - 1)];
    xyz[3 * ip + 1] = q[3 * (ip - 1) + 1];
    xyz[3 * ip + 2] = q[3 * (ip - 1) + 2];
    for (int j = 0; j < S; j++) sol[ip * S + j] = out[(ip - 1) * S + j];
    if (ptag) ptag[ip] = qtag[ip - 1];
  }
}
static void launch_promote(const double *q, const double *out, const uint16_t *qtag, int64_t n, int S, double *xyz,
                           double *sol, uint16_t *ptag, hipStream_t s) {
  hipLaunchKernelGGL(k_promote, dim3(pmx_grid(n + 1, 16384)), dim3(256), 0, s, q, out, qtag, n, S, xyz, sol, ptag);
}
// rows the step did not write (not located, frozen, failed): the caller's
// values, uploaded as (row, offset, size) + 6 doubles
__global__ __launch_bounds__(256) void k_patch_rows(const int4 *__restrict__ ent, const double *__restrict__ vals,
                                                    int64_t n, int S, double *__restrict__ sol) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int4 e = ent[i];                       // x: vertex, y: offset, z: size
    for (int j = 0; j < e.z; j++) sol[(int64_t)e.x * S + e.y + j] = vals[6 * i + j];
  }
}
void launch_patch_rows(const int4 *ent, const double *vals, int64_t n, int S, double *sol, hipStream_t s) {
  if (n < 1) return;
  hipLaunchKernelGGL(k_patch_rows, dim3(pmx_grid(n, 4096)), dim3(256), 0, s, ent, vals, n, S, sol);
}

// a split group as the background (pmx_split_adopt): xyz[i] / sol[i] = row
// idx[i - 1] of sxyz / ssol for i = 1..n, row 0 zeroed (S = 0: sol is not touched).
// One thread per 8-byte word of the destination, xyz's 3 (n + 1) words first,
// then sol's S (n + 1): word t is stored at t, so a wave stores 512 contiguous
// bytes, and the words of one source row are read by adjacent lanes.  idx is
// a first-visit numbering: mostly ascending, so neighbouring rows share lines.
__global__ __launch_bounds__(256) void k_gather_rows(const int *__restrict__ idx, int64_t n,
                                                     const double *__restrict__ sxyz,
                                                     const double *__restrict__ ssol, int S,
                                                     double *__restrict__ xyz, double *__restrict__ sol) {
  const int64_t nx = 3 * (n + 1), nw = nx + (int64_t)S * (n + 1);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nw; t += (int64_t)gridDim.x * blockDim.x) {
    if (t < nx) {
      const int64_t i = t / 3;
      const int c = (int)(t - 3 * i);
      xyz[t] = i ? sxyz[3 * (int64_t)idx[i - 1] + c] : 0.0;
    } else {
      const int64_t u = t - nx, i = u / S;
      const int c = (int)(u - S * i);
      sol[u] = i ? ssol[(int64_t)S * idx[i - 1] + c] : 0.0;
    }
  }
}
static void launch_gather_rows(const int *idx, int64_t n, const double *sxyz, const double *ssol, int S, double *xyz,
                               double *sol, hipStream_t s) {
  const int64_t nw = (int64_t)(3 + S) * (n + 1);
  hipLaunchKernelGGL(k_gather_rows, dim3(pmx_grid(nw, 1 << 20)), dim3(256), 0, s, idx, n, sxyz, ssol, S, xyz, sol);
}

// Mmg-layout trias (3 (nt + 1) ints) and adjt (3 nt + 4 ints) on the device ->
// TriRec records 0..nt, record 0 zeroed; an entry outside the range the host's
// staging accepts (vertex 1..np, adjt >= 0, adjt / 3 <= nt) counts into *bad.
// One thread per tria: its 3 vertices and 3 adjt entries in, one 32-B record
// out (two 16-B stores, consecutive lanes consecutive records).  The ranges
// are stage_trias'.
__global__ __launch_bounds__(256) void k_tri_records(const int *__restrict__ tria, const int *__restrict__ adjt,
                                                     int64_t nt, int64_t np, TriRec *__restrict__ tris,
                                                     unsigned *__restrict__ bad) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nt;
       k += (int64_t)gridDim.x * blockDim.x) {
    int4 v = make_int4(0, 0, 0, 0), nb = make_int4(0, 0, 0, 0);
    if (k) {
      const int a0 = adjt[3 * (k - 1) + 1], a1 = adjt[3 * (k - 1) + 2], a2 = adjt[3 * (k - 1) + 3];
      v = make_int4(tria[3 * k], tria[3 * k + 1], tria[3 * k + 2], 0);
      nb = make_int4(a0 / 3, a1 / 3, a2 / 3, 0);
      if (v.x < 1 || v.x > np || v.y < 1 || v.y > np || v.z < 1 || v.z > np || a0 < 0 || a1 < 0 || a2 < 0 ||
          nb.x > nt || nb.y > nt || nb.z > nt)
        atomicAdd(bad, 1u);
    }
    int4 *r = reinterpret_cast<int4 *>(tris + k);
    r[0] = v;
    r[1] = nb;
  }
}
static void launch_tri_records(const int *tria, const int *adjt, int64_t nt, int64_t np, TriRec *tris, unsigned *bad,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_tri_records, dim3(pmx_grid(nt + 1, 1 << 20)), dim3(256), 0, s, tria, adjt, nt, np, tris, bad);
}

namespace {

bool check_background(const pmx_call &C, const pmx_mesh_view *m, int nsol, const pmx_sol_view *sols, int imet) {
  if (m->np < 1 || m->ne < 1 || m->nt < 0 || m->np >= (1LL << 31) - 1 || 4 * m->ne >= (1LL << 31))
    return C.fail("mesh sizes out of range");
  if (!m->point_c || !m->tetra_v || m->point_stride < 24 || m->tetra_stride < 16)
    return C.fail("point_c / tetra_v missing or strides too small");
  if (nsol < 0 || nsol > PMX_MAX_SOLS || imet < -1 || imet >= nsol || (nsol > 0 && !sols))
    return C.fail("bad solution list");
  for (int s = 0; s < nsol; s++) {
    if (sols[s].size != 1 && sols[s].size != 3 && sols[s].size != 6) return C.fail("solution size must be 1, 3 or 6");
    if (!sols[s].m) return C.fail("null solution");
  }
  if (m->nt > 0 && (!m->tria_v || !m->adjt || m->tria_stride < 12)) return C.fail("nt > 0 requires tria_v and adjt");
  return true;
}

// the interleaved row layout of nsol solutions: offsets and row width
SolDesc make_sol_desc(int nsol, int imet, const pmx_sol_view *sols) {
  SolDesc sd{};
  sd.nsol = nsol;
  sd.imet = imet;
  for (int s = 0; s < nsol; s++) {
    sd.size[s] = sols[s].size;
    sd.off[s] = sd.S;
    sd.S += sols[s].size;
  }
  return sd;
}

// boundary triangles of a mesh view -> TriRec records, validated against np
bool stage_trias(pmx_ctx *ctx, const pmx_mesh_view *m, int64_t np, std::vector<TriRec> &htr) {
  const int64_t nt = m->nt;
  htr.assign((size_t)(nt + 1), TriRec{});
  if (nt < 1) return true;
  const char *rc = (const char *)m->tria_v;
  for (int64_t k = 1; k <= nt; k++) {
    const int *v = (const int *)(rc + k * m->tria_stride);
    TriRec &r = htr[(size_t)k];
    for (int l = 0; l < 3; l++) {
      r.v[l] = v[l];
      const int a = m->adjt[3 * (k - 1) + 1 + l];
      r.nb[l] = a / 3;
      if (v[l] < 1 || v[l] > np || a < 0 || a / 3 > nt) {
        ctx->err = "tria vertex or adjacency index out of range";
        return false;
      }
    }
  }
  return true;
}

// the volume hint grid over the background bbox [lo, hi] (about one cell per
// 6 tets) and the surface (tria) grid
bool setup_grids(pmx_ctx *ctx, const double lo[3], const double hi[3], int64_t ne) {
  double ext[3], vol = 1.0;
  for (int a = 0; a < 3; a++) {
    ext[a] = std::max(hi[a] - lo[a], 1e-300);
    vol *= ext[a];
  }
  double target = std::max(1.0, (double)ne / 6.0);
  double h = std::cbrt(vol / target);
  GridDesc g;
  int64_t cells = 1;
  for (int a = 0; a < 3; a++) {
    // 1e-9 slack: libm cbrt is not correctly rounded, and 255.00000000000003
    // cells must stay 255 (r01: C3 got 256 per axis, misaligned with the
    // mesh: 10% empty cells, 0.73 instead of 0.44 cells start distance)
    int d = (int)std::ceil(ext[a] / h * (1.0 - 1e-9));
    d = std::max(1, std::min(d, 4096));
    g.dim[a] = d;
    int bits = 0;
    while ((1 << bits) < d) bits++;
    g.qf[a] = 21 - bits;
    g.lo[a] = lo[a];
    g.inv[a] = (double)d / ext[a];
    cells *= d;
  }
  ctx->grid = g;
  ctx->gcells = cells;
  for (int a = 0; a < 3; a++) { ctx->bblo[a] = lo[a]; ctx->bbhi[a] = hi[a]; }
  if (!ctx->size_tria_grid()) return false;
  return pmx_dgrow(ctx, ctx->d_grid, (size_t)cells);
}

// the background's derived layouts, decided per upload / adoption (A/B
// switches): PMX_WALK_RECORDS=compact builds the
// walk's 24-B records (a device pass per background: 1.26 ms at C3 for a walk
// 2 % faster); PMX_HINT_SAMPLE_ORDER=2 the vertex-owner hint sample (three
// device passes per background, 1.26 ms at C3, for a hint build 0.03 ms
// faster on a lexicographic numbering).  Defaults: neither -- no device pass
// per background beyond what every step does.
bool env_compact_records() {
  const char *e = getenv("PMX_WALK_RECORDS");
  return e && strcmp(e, "compact") == 0;
}
int env_sample_mode() {
  const char *e = getenv("PMX_HINT_SAMPLE_ORDER");
  return (e && atoi(e) == 2) ? 2 : 0;
}

// ---- the install path: begin, grow, (the caller's transfers), finish -----------

// Whatever happens after this, the context holds no usable background until
// finish_background has completed: a failed install must not leave sizes that
// disagree with the device buffers.  Every flag of data derived from the
// background belongs here and nowhere else (the merge plan does not: it is
// independent of the background).  layout_env: the records' layout is decided
// again (a promotion keeps the one its residency build was made for).
void begin_background(pmx_ctx *ctx, bool layout_env) {
  ctx->have_bg = ctx->ran = ctx->have_derived = ctx->have_tetv = ctx->have_qual = false;
  ctx->have_pmap = ctx->split_valid = ctx->moveifc_valid = false;
  pmx_part_drop(ctx);
  ctx->have_ptag = ctx->have_csr = ctx->have_surf = ctx->fan_rot = ctx->bg_btv = false;
  ctx->stat_np = -1;
  ctx->eager_nch = 0;
  ctx->h_nbad.p[PMX_H_BAD_TRIAS] = 0;     // only an adopt with a surface counts any
  if (layout_env) {
    ctx->compact_recs = env_compact_records();
    ctx->sample_mode = env_sample_mode();
  }
}

// the tria-sized part of the chain below, on its own for the installer that
// learns nt on the device (an adopt with a surface calls it a second time)
bool grow_trias(pmx_ctx *ctx, int64_t nt) {
  return pmx_dgrow(ctx, ctx->d_tris, (size_t)(nt + 1)) && pmx_dgrow(ctx, ctx->d_trn, (size_t)(nt + 1));
}

// the background's device arrays for np vertices, ne tets, nt trias and rows
// of S doubles; btv: the connectivity goes to d_btv and the device matches
// its faces (d_adja grown here, before any copy is in flight)
bool grow_background(pmx_ctx *ctx, int64_t np, int64_t ne, int64_t nt, int S, bool btv) {
  const int64_t ns = (ne + PMX_HINT_STRIDE - 1) / PMX_HINT_STRIDE;
  return pmx_dgrow(ctx, ctx->d_xyz, (size_t)(np + 1) * 3) && pmx_dgrow(ctx, ctx->d_tets, (size_t)(ne + 1)) &&
         (!ctx->compact_recs || pmx_dgrow(ctx, ctx->d_wrec, (size_t)(ne + 1))) &&
         pmx_dgrow(ctx, ctx->d_wfar, PMX_D_WORDS) && pmx_dgrow(ctx, ctx->d_tets_s, (size_t)std::max<int64_t>(ns, 1)) &&
         pmx_dgrow(ctx, ctx->d_sol, (size_t)(np + 1) * std::max(S, 1)) && grow_trias(ctx, nt) &&
         pmx_dgrow(ctx, ctx->d_xyzq, (size_t)(np + 1)) &&
         (!btv || (pmx_dgrow(ctx, ctx->d_btv, (size_t)(ne + 1)) && pmx_dgrow(ctx, ctx->d_adja, (size_t)(4 * ne + 5))));
}

// what an installer hands to finish_background
struct BgTail {
  int64_t np, ne, nt;
  double hausd;
  const double *lo, *hi;                 // bounding box
  const std::vector<TriRec> *trias;      // the host's trias, sent here (nullptr: d_tris is set)
  bool btv;                              // the records were built from d_btv (a FRESH step rebuilds them)
  bool sample;                           // the owner sample is still to be queued (false: the caller did)
  hipEvent_t join;                       // records built on another stream: joined before the sync
};

// The common tail on the call's stream: sizes, grids, owner sample, trias, fan
// check, one sync, the non-manifold check; the background is usable after it.
// (The node -> trias fans are the step's: PMMG_precompute_nodeTrias runs
// inside the reference's call.)
bool finish_background(const pmx_call &C, const BgTail &t, Trace &tr) {
  pmx_ctx *ctx = C.ctx;
  ctx->np = t.np; ctx->ne = t.ne; ctx->nt = t.nt; ctx->hausd = t.hausd;
  if (!setup_grids(ctx, t.lo, t.hi, t.ne)) return false;
  if (t.sample && !ctx->order_hint_samples(t.ne, t.np, C.s)) return false;
  tr.mark("grids");
  if (t.trias)
    PMX_CK(C, hipMemcpyAsync(ctx->d_tris.p, t.trias->data(), t.trias->size() * sizeof(TriRec), hipMemcpyHostToDevice, C.s));
  if (!ctx->check_fans(C.s)) return false;
  if (t.join) PMX_CK(C, hipStreamWaitEvent(C.s, t.join, 0));
  PMX_CK(C, hipGetLastError());
  tr.mark("trias + topology");
  PMX_CK(C, hipStreamSynchronize(C.s));   // the caller's host staging dies after this
  tr.mark("sync");
  if (ctx->h_nbad.p[PMX_H_NONMANIFOLD]) return C.fail("non-manifold tet faces");
  if (ctx->h_nbad.p[PMX_H_BAD_TRIAS]) return C.fail("tria vertex or adjacency index out of range");
  ctx->fan_rot = ctx->nt > 0 && ctx->h_nbad.p[PMX_H_BAD_FANS] == 0;
  ctx->nsamp = ctx->samples_owner ? (int64_t)ctx->h_nbad.p[PMX_H_NSAMP] : 0;
  ctx->bg_btv = t.btv;
  ctx->have_bg = true;
  return true;
}

}  // namespace

// ---- tet records -----------------------------------------------------------------

// tv == nullptr: dst's 32-B records are in place (the host packed them); only
// the compact records are built.  d_adja and the face matching's scratch are
// shared by the builds on the main and the topo stream (an upload, a FRESH
// step's rederive, the residency build): each build waits for the one before
// it in enqueue order and records ev_adja once it no longer reads them.
bool pmx_ctx::build_records(const int4 *tv, const int *host_adja, int64_t ne, int64_t np, const RecordSet &dst,
                            hipStream_t s) {
  const pmx_call C{this, "tet records", s};
  const int64_t ns = (ne + PMX_HINT_STRIDE - 1) / PMX_HINT_STRIDE;
  if (!pmx_dgrow(this, *dst.tets, (size_t)(ne + 1)) || (compact_recs && !pmx_dgrow(this, *dst.wrec, (size_t)(ne + 1))) ||
      !pmx_dgrow(this, d_wfar, PMX_D_WORDS) || !pmx_dgrow(this, *dst.sample, (size_t)std::max<int64_t>(ns, 1)))
    return false;
  if (!tv || host_adja) h_nbad.p[dst.h_nonmanifold] = 0;   // no face matching
  if (tv) {
    if (!pmx_dgrow(this, d_adja, (size_t)(4 * ne + 5))) return false;
    if (ev_adja.e) PMX_CK(C, hipStreamWaitEvent(s, ev_adja, 0));
    if (host_adja)
      PMX_CK(C, hipMemcpyAsync(d_adja.p, host_adja, (size_t)(4 * ne + 5) * sizeof(int), hipMemcpyHostToDevice, s));
    else if (!pmx_ctx_build_adja_device(this, tv, ne, np, d_adja.p, s, h_nbad.p + dst.h_nonmanifold))
      return false;
    launch_build_tetrec(tv, d_adja.p, ne, PMX_HINT_STRIDE, dst.tets->p, dst.sample->p, s);
    if (!ev_adja.create(false)) return C.fail("creating the adjacency event");
    PMX_CK(C, hipEventRecord(ev_adja, s));
  }
  if (compact_recs) launch_build_wrec(dst.tets->p, ne, dst.wrec->p, d_wfar.p + dst.d_far, h_nbad.p + dst.h_far, s);
  else h_nbad.p[dst.h_far] = 0;                            // no far fields unless compact records are built
  return true;
}

// The hint sample, once the tets are on the device and np set
// (sample_mode, PMX_HINT_SAMPLE_ORDER at the upload): 0 every 4th tet in tet
// order, packed with the tet records (nothing to do here); 2 one tet per
// vertex, in vertex order (k_vmin_owner; its count lands in h_nbad[PMX_H_NSAMP],
// nsamp after the upload's sync) -- A/Bs in DESIGN.md section 7 r05 / r06.  (r05's
// mode 1, the every-4th-tet sample sorted by smallest vertex, was dropped in
// r06: its sort could not be redone by a FRESH step.)
bool pmx_ctx::order_hint_samples(int64_t ne, int64_t np, hipStream_t s) {
  samples_sorted = samples_owner = false;
  if (sample_mode != 2 || np < 1 || ne < 1) return true;
  const size_t tb = owner_scan_temp_bytes(np);
  if (!pmx_dgrow(this, d_skey, (size_t)(np + 2)) || !pmx_dgrow(this, d_sidx, (size_t)(2 * (np + 1))) ||
      !pmx_dgrow(this, d_salt, (size_t)(np + 1)) || !pmx_dgrow(this, d_tets_sk, (size_t)(np + 1)) ||
      !pmx_dgrow(this, d_stmp, std::max<size_t>(tb, 1)) || !pmx_dgrow(this, d_wfar, PMX_D_WORDS))
    return false;
  if (!launch_owner_sample(d_tets.p, ne, np, d_skey.p, d_sidx.p, d_sidx.p + (np + 1), d_salt.p, d_tets_sk.p,
                           d_wfar.p + PMX_D_NSAMP, h_nbad.p + PMX_H_NSAMP, d_stmp.p, tb, s)) {
    err = "hint sample: vertex owners";
    return false;
  }
  std::swap(d_tets_s, d_salt);
  samples_sorted = samples_owner = true;
  return true;
}

// PMX_RUN_FRESH_BACKGROUND: the device passes an upload runs on the raw
// arrays, again, in stream order on s -- a ParMmg iteration brings a new
// background (PMMG_update_oldGrps, src/libparmmg1.c:653) and the reference
// recomputes its derived data inside the call (src/interpmesh_pmmg.c:514-518):
// the face matching of the uploaded connectivity with the tet records and the
// every-4th-tet sample (MMG3D_hashTetra's adjacency on the device) when the
// device built them, the compact records, the owner sample
bool pmx_ctx::rederive(hipStream_t s) {
  if (!build_records(bg_btv ? d_btv.p : nullptr, nullptr, ne, np, records_current(), s)) return false;
  if (sample_mode == 2 && !order_hint_samples(ne, np, s)) return false;
  return pmx_call{this, "pmx_run", s}.hip(hipGetLastError(), "background records");
}

// ---- the three installers ----------------------------------------------------------

extern "C" {

int pmx_upload_background(pmx_ctx *ctx, const pmx_mesh_view *m, int nsol,
                          const pmx_sol_view *sols, int imet) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_upload_background", ctx->stream};
  begin_background(ctx, true);
  if (!m) return C.fail("null mesh");
  hipSetDevice(ctx->device);
  if (!check_background(C, m, nsol, sols, imet)) return 0;
  const int64_t np = m->np, ne = m->ne, nt = m->nt;
  const bool dev_adja = m->adja == nullptr;   // no MMG3D_hashTetra on the host: device face matching
  // the host packs the every-4th-tet hint sample with the tet records (the
  // device-adjacency path: k_build_tetrec writes it)
  const bool host_sample = !dev_adja && ctx->sample_mode == 0;
  Trace tr("background");
  const SolDesc sd = make_sol_desc(nsol, imet, sols);
  const int S = sd.S;
  const int64_t ns = (ne + PMX_HINT_STRIDE - 1) / PMX_HINT_STRIDE;
  const size_t hs_n = (size_t)(np + 1) * std::max(S, 1);
  // pinned staging: xyz | tets (TetRec, or int4 when the device builds the
  // adjacency) | packed hint sample | solutions; each part goes down as soon
  // as it is packed (the tets in chunks), one sync at the end
  const size_t trec = dev_adja ? sizeof(int4) : sizeof(TetRec);
  const size_t o_p = 0, o_t = o_p + pmx_call::al256((size_t)(np + 1) * 24),
               o_h = o_t + pmx_call::al256((size_t)(ne + 1) * trec),
               o_s = o_h + pmx_call::al256(host_sample ? (size_t)ns * sizeof(int4) : 0),
               total = o_s + pmx_call::al256(hs_n * sizeof(double));
  PMX_CK(C, hipStreamSynchronize(ctx->stream));   // the arena may still feed an earlier copy
  char *stg = pmx_hstage(ctx, total);
  if (!stg) return 0;
  // any return after the topology fork first waits for that stream (a later
  // call may regrow the buffers its kernels use)
  struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) hipStreamSynchronize(s); }
  } topo_guard;
  if (!grow_background(ctx, np, ne, nt, S, dev_adja)) return 0;
  hipStream_t st = ctx->stream;

  // points -> dense xyz (24 B), bounding box per chunk
  double *hp = (double *)(stg + o_p);
  hp[0] = hp[1] = hp[2] = 0.0;
  const char *pc = (const char *)m->point_c;
  double blo[64][3], bhi[64][3];
  const int nch = par_chunks(1, np + 1, [&](int c, int64_t i0, int64_t i1) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int64_t i = i0; i < i1; i++) {
      const double *cc = (const double *)(pc + i * m->point_stride);
      for (int a = 0; a < 3; a++) {
        hp[3 * i + a] = cc[a];
        lo[a] = std::min(lo[a], cc[a]);
        hi[a] = std::max(hi[a], cc[a]);
      }
    }
    for (int a = 0; a < 3; a++) { blo[c][a] = lo[a]; bhi[c][a] = hi[a]; }
  });
  double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (int c = 0; c < nch; c++)
    for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], blo[c][a]); hi[a] = std::max(hi[a], bhi[c][a]); }
  PMX_CK(C, hipMemcpyAsync(ctx->d_xyz.p, hp, (size_t)(np + 1) * 24, hipMemcpyHostToDevice, st));
  tr.mark("points");
  // tets -> TetRec with neighbour tet index (or the bare connectivity), + the
  // packed hint sample (the connectivity of every PMX_HINT_STRIDE-th tet,
  // contiguous: the hint build streams ne/4 * 16 B instead of touching every
  // line of the tet records); in chunks, each DMA'd while the next is packed
  TetRec *ht = (TetRec *)(stg + o_t);
  int4 *htv = (int4 *)(stg + o_t);
  int4 *hh = (int4 *)(stg + o_h);
  if (dev_adja) htv[0] = make_int4(0, 0, 0, 0);
  else memset(&ht[0], 0, sizeof(TetRec));
  const char *tc = (const char *)m->tetra_v;
  const int *adja_in = m->adja;
  bool bad = false;
  const int64_t ntc = std::max<int64_t>(1, std::min<int64_t>(8, ne >> 20));
  for (int64_t c = 0; c < ntc; c++) {
    const int64_t klo = (c == 0) ? 0 : 1 + ne * c / ntc, khi = 1 + ne * (c + 1) / ntc;
    par_for(std::max<int64_t>(klo, 1), khi, [&](int64_t k0, int64_t k1) {
      bool b = false;
      for (int64_t k = k0; k < k1; k++) {
        const int *v = (const int *)(tc + k * m->tetra_stride);
        // indices the kernels will gather through: a valid tet (v[0] > 0,
        // MG_EOK) must name vertices 1..np and neighbours 0..ne
        const bool valid = v[0] > 0;
        if (dev_adja) {
          if (!valid) { st4(&htv[k], 0, 0, 0, 0); }
          else {
            for (int l = 0; l < 4; l++)
              if (v[l] < 1 || v[l] > np) b = true;
            st4(&htv[k], v[0], v[1], v[2], v[3]);
          }
        } else {
          TetRec &r = ht[(size_t)k];
          for (int l = 0; l < 4; l++) {
            r.v[l] = v[l];
            const int a = adja_in[4 * (k - 1) + 1 + l];
            r.nb[l] = a / 4;
            if (valid && (v[l] < 1 || v[l] > np || a < 0 || a / 4 > ne)) b = true;
          }
        }
        if (host_sample && (k - 1) % PMX_HINT_STRIDE == 0)
          hh[(k - 1) / PMX_HINT_STRIDE] = make_int4(v[0], v[1], v[2], v[3]);
      }
      if (b) __atomic_store_n(&bad, true, __ATOMIC_RELAXED);
      std::atomic_thread_fence(std::memory_order_seq_cst);
    });
    if (bad) break;
    if (dev_adja)
      PMX_CK(C, hipMemcpyAsync(ctx->d_btv.p + klo, htv + klo, (size_t)(khi - klo) * sizeof(int4), hipMemcpyHostToDevice, st));
    else
      PMX_CK(C, hipMemcpyAsync(ctx->d_tets.p + klo, ht + klo, (size_t)(khi - klo) * sizeof(TetRec), hipMemcpyHostToDevice, st));
  }
  if (bad) return C.fail("tet vertex or adjacency index out of range");
  // the records (the host's: only their compact copy) and the owner sample
  // (mode 2) while the host packs the solutions and trias.  With the device's
  // face matching they run on the topology stream as soon as the connectivity
  // is down, overlapping that packing and its DMA; joined before the final sync
  hipStream_t rs = st;
  if (dev_adja) {
    PMX_CK(C, hipEventRecord(ctx->ev_fork, st));
    PMX_CK(C, hipStreamWaitEvent(ctx->topo, ctx->ev_fork, 0));
    topo_guard.s = rs = ctx->topo;
  } else if (host_sample) {
    PMX_CK(C, hipMemcpyAsync(ctx->d_tets_s.p, hh, (size_t)ns * sizeof(int4), hipMemcpyHostToDevice, st));
  }
  if (!ctx->build_records(dev_adja ? ctx->d_btv.p : nullptr, nullptr, ne, np, ctx->records_current(), rs) ||
      !ctx->order_hint_samples(ne, np, rs))
    return 0;
  if (dev_adja) PMX_CK(C, hipEventRecord(ctx->ev_join, ctx->topo));
  tr.mark("tets");
  // solutions -> interleaved [np+1][S], in blocks of 1024 rows (each row's
  // line written while it is in cache, not once per solution) and chunks
  // whose DMA overlaps the packing of the next
  double *hs = (double *)(stg + o_s);
  // row 0: Mmg's unused slot, as the caller holds it (no kernel reads a
  // vertex 0 -- but PMMG_prilen's parallel edges with a tensor metric and
  // metRidTyp = 1 read met->m[ip] flat, src/quality_pmmg.c:466, i.e. row 0
  // for ip < 6)
  memset(hs, 0, (size_t)std::max(S, 1) * sizeof(double));
  for (int s = 0; s < nsol; s++)
    for (int j = 0; j < sols[s].size; j++) hs[sd.off[s] + j] = sols[s].m[j];
  if (S == 0) {
    memset(hs, 0, hs_n * sizeof(double));
    PMX_CK(C, hipMemcpyAsync(ctx->d_sol.p, hs, hs_n * sizeof(double), hipMemcpyHostToDevice, st));
  } else {
    const int64_t nsc = std::max<int64_t>(1, std::min<int64_t>(4, (np * S) >> 21));
    for (int64_t c = 0; c < nsc; c++) {
      const int64_t r0 = (c == 0) ? 0 : 1 + np * c / nsc, r1 = 1 + np * (c + 1) / nsc;
      par_for(std::max<int64_t>(r0, 1), r1, [&](int64_t i0, int64_t i1) {
        for (int64_t b0 = i0; b0 < i1; b0 += 1024) {
          const int64_t b1 = std::min(i1, b0 + 1024);
          for (int s = 0; s < nsol; s++) {
            const int sz = sols[s].size, off = sd.off[s];
            const double *src = sols[s].m;
            for (int64_t i = b0; i < b1; i++)
              for (int j = 0; j < sz; j++) hs[(size_t)i * S + off + j] = src[i * sz + j];
          }
        }
      });
      PMX_CK(C, hipMemcpyAsync(ctx->d_sol.p + r0 * S, hs + r0 * S, (size_t)((r1 - r0) * S) * sizeof(double),
                               hipMemcpyHostToDevice, st));
    }
  }
  tr.mark("solutions");
  // boundary triangles
  std::vector<TriRec> htr;
  if (!stage_trias(ctx, m, np, htr)) return 0;
  ctx->sd = sd;
  return finish_background(C, {np, ne, nt, m->hausd, lo, hi, &htr, dev_adja, false, dev_adja ? ctx->ev_join.e : nullptr}, tr);
}

// The last step's points, results and new tets become the background (device
// residency across ParMmg iterations, pmx_points.hip): only the boundary trias
// and the rows the step did not write come from the host.

int pmx_promote_background(pmx_ctx *ctx, const pmx_mesh_view *m, int nsol, const pmx_sol_view *sols) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_promote_background", ctx->stream};
  if (!m) return C.fail("null mesh");
  if (!ctx->stepped() || ctx->out_S != ctx->sd.S) return C.fail("no step has run on the current uploads");
  if (!ctx->ntets.have) return C.fail("upload the new tets first");
  if (ctx->pts_first != 1) return C.fail("the points view must start at 1 (Mmg numbering)");
  const int64_t n = ctx->nq, ne = ctx->ntets.n, nt = m->nt;
  if (m->np != n || m->ne != ne || n < 1) return C.fail("mesh sizes differ from the uploaded points / new tets");
  if (nt < 0 || (nt > 0 && (!m->tria_v || !m->adjt || m->tria_stride < 12)))
    return C.fail("nt > 0 requires tria_v and adjt");
  const SolDesc sd = ctx->sd;
  if (nsol != sd.nsol || (nsol > 0 && !sols)) return C.fail("solution list differs from the step's");
  for (int s = 0; s < nsol; s++)
    if (sols[s].size != sd.size[s]) return C.fail("solution size differs from the step's");
  if (m->adja) {
    // the walks gather through these: every neighbour of a valid tet must
    // name a face of 1..ne (as pmx_upload_background checks)
    bool badj = false;
    par_chunks(1, ne + 1, [&](int, int64_t k0, int64_t k1) {
      bool b = false;
      for (int64_t k = k0; k < k1 && !b; k++) {
        if (m->tetra_v && *(const int *)((const char *)m->tetra_v + k * m->tetra_stride) <= 0) continue;
        for (int f = 0; f < 4; f++) {
          const int a = m->adja[4 * (k - 1) + 1 + f];
          if (a < 0 || a / 4 > ne) b = true;
        }
      }
      if (b) __atomic_store_n(&badj, true, __ATOMIC_RELAXED);
    });
    if (badj) return C.fail("adjacency entry out of range");
  }
  hipSetDevice(ctx->device);
  Trace tr("promote");
  hipStream_t st = ctx->stream;
  if (!ctx->ntets.fix_orphans() || !ctx->ntets.ensure_tets(st)) return 0;
  PMX_CK(C, hipStreamSynchronize(st));
  if (!ctx->check_device_errors()) return 0;
  tr.mark("sync");
  const int S = sd.S;
  // rows the step did not write keep the caller's values (Mmg's own, or the
  // frozen-point copy): which ones, from the write masks
  char *stg = pmx_hstage(ctx, (size_t)n);
  if (!stg) return 0;
  PMX_CK(C, hipMemcpyAsync(stg, ctx->d_wmask.p, (size_t)n, hipMemcpyDeviceToHost, st));
  PMX_CK(C, hipStreamSynchronize(st));
  const uint8_t *wm = (const uint8_t *)stg;
  const unsigned full = (1u << nsol) - 1u;
  // per chunk, then concatenated in chunk order
  std::vector<std::vector<int4>> cent(64);
  std::vector<std::vector<double>> cval(64);
  bool missing = false;
  const int nch = par_chunks(0, n, [&](int c, int64_t j0, int64_t j1) {
    for (int64_t j = j0; j < j1; j++) {
      if ((wm[j] & full) == full) continue;      // every solution written (the common case)
      for (int s = 0; s < nsol; s++) {
        if (wm[j] & (1u << s)) continue;
        const int sz = sd.size[s];
        if (!sols[s].m) { __atomic_store_n(&missing, true, __ATOMIC_RELAXED); continue; }
        cent[(size_t)c].push_back(make_int4((int)(j + 1), sd.off[s], sz, 0));
        const double *src = sols[s].m + j * sz;   // pmx_download's layout
        for (int q = 0; q < 6; q++) cval[(size_t)c].push_back(q < sz ? src[q] : 0.0);
      }
    }
  });
  if (missing) return C.fail("a row the step did not write needs the caller's solution");
  std::vector<int4> ent;
  std::vector<double> vals;
  for (int c = 0; c < nch; c++) {
    ent.insert(ent.end(), cent[(size_t)c].begin(), cent[(size_t)c].end());
    vals.insert(vals.end(), cval[(size_t)c].begin(), cval[(size_t)c].end());
  }
  tr.mark("unwritten rows");
  // boundary trias of the new mesh (the host's: Mmg's numbering)
  std::vector<TriRec> htr;
  if (!stage_trias(ctx, m, n, htr)) return 0;
  tr.mark("trias");
  // nothing has moved so far: a promotion refused above leaves the step
  // promotable.  From here on the background is invalid until this completes
  begin_background(ctx, false);
  if (!grow_background(ctx, n, ne, nt, S, false)) return 0;
  const bool tags = ctx->have_qtag;
  if (tags && !pmx_dgrow(ctx, ctx->d_ptag, (size_t)(n + 1))) return 0;
  launch_promote(ctx->d_qxyz.p, ctx->d_out.p, tags ? ctx->d_qtag.p : nullptr, n, S, ctx->d_xyz.p, ctx->d_sol.p,
                 tags ? ctx->d_ptag.p : nullptr, st);
  if (!ent.empty()) {
    if (!pmx_dgrow(ctx, ctx->d_pent, ent.size()) || !pmx_dgrow(ctx, ctx->d_pval, vals.size())) return 0;
    PMX_CK(C, hipMemcpyAsync(ctx->d_pent.p, ent.data(), ent.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    PMX_CK(C, hipMemcpyAsync(ctx->d_pval.p, vals.data(), vals.size() * sizeof(double), hipMemcpyHostToDevice, st));
    launch_patch_rows(ctx->d_pent.p, ctx->d_pval.p, (int64_t)ent.size(), S, ctx->d_sol.p, st);
  }
  tr.mark("promote launch");
  // tet records: the set prepared while the step ran (residency on) is swapped
  // in with its counts, once its build has finished -- else they are built
  // from the caller's Mmg adjacency (mesh->adja after remeshing) or from the
  // device's face matching (a residency build still running is then left to
  // finish behind ev_adja: its result is dropped)
  const bool prepared = ctx->ntets.take_next(!m->adja);
  if (prepared) {
    PMX_CK(C, hipEventSynchronize(ctx->ntets.ev_topo));
    tr.mark("wait topo");
    std::swap(ctx->d_tets, ctx->d_tets_next);
    std::swap(ctx->d_wrec, ctx->d_wrec_next);
    std::swap(ctx->d_tets_s, ctx->d_tets_s_next);
    ctx->h_nbad.p[PMX_H_NONMANIFOLD] = ctx->h_nbad.p[PMX_H_NONMANIFOLD_NEXT];
    ctx->h_nbad.p[PMX_H_FAR] = ctx->h_nbad.p[PMX_H_FAR_NEXT];
  } else if (!ctx->build_records(ctx->ntets.d_v.p, m->adja, ne, n, ctx->records_current(), st)) {
    return 0;
  }
  tr.mark("tet records");
  // (records from the new tets or the caller's adja, not d_btv: a FRESH step keeps them)
  if (!finish_background(C, {n, ne, nt, m->hausd, ctx->qlo, ctx->qhi, &htr, false, true, nullptr}, tr)) return 0;
  ctx->have_ptag = tags;
  // the points and the results were consumed: the next step needs new points
  ctx->have_pts = ctx->ran = false;
  ctx->ntets.consumed();
  return 1;
}

}  // extern "C"

namespace {
struct Axis {
  const double *xyz;
  int a;
  __device__ double operator()(const int &i) const { return xyz[3 * ((int64_t)i + 1) + a]; }
};
}  // namespace

bool pmx_bbox_device(const pmx_call &C, const double *xyz, int64_t np, DevBuf<double> &bb, DevBuf<char> &tmp,
                     double lo[3], double hi[3]) {
  if (!C.grow(bb, 6)) return false;
  hipcub::CountingInputIterator<int> it(0);
  for (int a = 0; a < 3; a++) {
    hipcub::TransformInputIterator<double, Axis, hipcub::CountingInputIterator<int>> in(it, Axis{xyz, a});
    size_t b = 0;
    hipcub::DeviceReduce::Min(nullptr, b, in, bb.p + a, (int)np, C.s);
    if (!C.grow(tmp, b) || !C.ok(hipcub::DeviceReduce::Min(tmp.p, b, in, bb.p + a, (int)np, C.s), "bbox"))
      return false;
    hipcub::DeviceReduce::Max(nullptr, b, in, bb.p + 3 + a, (int)np, C.s);
    if (!C.grow(tmp, b) || !C.ok(hipcub::DeviceReduce::Max(tmp.p, b, in, bb.p + 3 + a, (int)np, C.s), "bbox"))
      return false;
  }
  double h[6];
  if (!C.read_words(h, (const double *)bb.p, 6, "bbox")) return false;
  for (int a = 0; a < 3; a++) { lo[a] = h[a]; hi[a] = h[3 + a]; }
  return true;
}

// A device-resident group as the background (pmx_merge_adopt, pmx_split_adopt):
// pmx_upload_background's device-adjacency path, its host packing and DMA
// replaced by device-to-device copies or a row gather, its host trias by none
// (nt = 0) or by the boundary build on the records' neighbour fields
bool pmx_ctx_adopt_group(pmx_ctx *ctx, const char *who, const AdoptSrc &src, const SolDesc &sd, int64_t np,
                         int64_t ne) {
  const pmx_call C{ctx, who, ctx->stream};
  begin_background(ctx, true);
  if (np < 1 || ne < 1 || np >= (1LL << 31) - 1 || 4 * ne >= (1LL << 31)) return C.fail("mesh sizes out of range");
  if (!grow_background(ctx, np, ne, 0, sd.S, true)) return false;
  hipStream_t st = ctx->stream;
  const size_t hs_n = (size_t)(np + 1) * std::max(sd.S, 1);
  if (src.idx) {
    launch_gather_rows(src.idx, np, src.xyz, src.sol, sd.S, ctx->d_xyz.p, ctx->d_sol.p, st);
    if (sd.S == 0 && !C.hip(hipMemsetAsync(ctx->d_sol.p, 0, hs_n * sizeof(double), st), "solutions")) return false;
  } else if (!C.hip(hipMemcpyAsync(ctx->d_xyz.p, src.xyz, (size_t)(np + 1) * 24, hipMemcpyDeviceToDevice, st), "points") ||
             !C.hip(sd.S > 0 ? hipMemcpyAsync(ctx->d_sol.p, src.sol, hs_n * sizeof(double), hipMemcpyDeviceToDevice, st)
                             : hipMemsetAsync(ctx->d_sol.p, 0, hs_n * sizeof(double), st), "solutions")) {
    return false;
  }
  if (!C.hip(hipMemsetAsync(ctx->d_btv.p, 0, sizeof(int4), st), "tets") ||
      !C.hip(hipMemcpyAsync(ctx->d_btv.p + 1, src.tv, (size_t)ne * sizeof(int4), hipMemcpyDeviceToDevice, st), "tets") ||
      !C.hip(hipMemsetAsync(ctx->d_tris.p, 0, sizeof(TriRec), st), "trias"))
    return false;
  if (!ctx->build_records(ctx->d_btv.p, nullptr, ne, np, ctx->records_current(), st)) return false;
  ctx->sd = sd;
  Trace tr("adopt");
  double lo[3], hi[3];
  if (!pmx_bbox_device(C, ctx->d_xyz.p, np, ctx->d_bb, ctx->d_bbtmp, lo, hi)) return false;
  tr.mark("copies + records + bbox");
  int64_t nt = 0;
  if (src.surface) {
    // the bbox's sync has brought the face matching's count: stop before a
    // surface is built on an adjacency that left shared faces at 0
    if (ctx->h_nbad.p[PMX_H_NONMANIFOLD]) return C.fail("non-manifold tet faces");
    // adja == 0 <=> the record's neighbour field is 0: d_adja itself stays build_records' alone
    if (!pmx_bdry_device(C, ctx->d_btv.p, reinterpret_cast<const int *>(ctx->d_tets.p), 8, 4, ne, np, true, 4 * ne,
                         ctx->bdry, &nt, nullptr, nullptr))
      return false;
    if (!grow_trias(ctx, nt)) return false;
    if (nt > 0) {
      unsigned *bad = ctx->d_wfar.p + PMX_D_BAD_TRIAS;
      if (!C.hip(hipMemsetAsync(bad, 0, sizeof(unsigned), st), "trias")) return false;
      launch_tri_records(ctx->bdry.tria.p, ctx->bdry.adjt.p, nt, np, ctx->d_tris.p, bad, st);
      if (!C.hip(hipMemcpyAsync(ctx->h_nbad.p + PMX_H_BAD_TRIAS, bad, sizeof(unsigned), hipMemcpyDeviceToHost, st), "trias"))
        return false;
    } else if (!C.hip(hipMemsetAsync(ctx->d_tris.p, 0, sizeof(TriRec), st), "trias")) {
      return false;
    }
    tr.mark("surface");
  }
  return finish_background(C, {np, ne, nt, src.surface ? src.hausd : 0.0, lo, hi, nullptr, true, true, nullptr}, tr);
}

extern "C" int64_t pmx_download_surface(pmx_ctx *ctx, int *tria, int64_t maxnt, int *adjt) {
  if (!ctx) return -1;
  const pmx_call C{ctx, "pmx_download_surface", ctx->stream};
  if (!ctx->have_bg) return C.fail("no background installed"), -1;
  const int64_t nt = ctx->nt;
  if (!tria) return nt;                          // the size query: nothing is copied
  if (nt > maxnt) return C.fail("more trias than maxnt"), -1;
  hipSetDevice(ctx->device);
  std::vector<TriRec> h((size_t)(nt + 1));
  if (!C.hip(hipMemcpyAsync(h.data(), ctx->d_tris.p, h.size() * sizeof(TriRec), hipMemcpyDeviceToHost, C.s), "download") ||
      !C.sync("download"))
    return -1;
  for (int64_t k = 1; k <= nt; k++)
    for (int l = 0; l < 3; l++) tria[3 * k + l] = h[(size_t)k].v[l];
  if (!adjt) return nt;
  // the records keep the neighbouring tria only: its edge is the one that
  // joins the same two vertices
  adjt[0] = adjt[3 * nt + 1] = adjt[3 * nt + 2] = adjt[3 * nt + 3] = 0;
  for (int64_t k = 1; k <= nt; k++) {
    const TriRec &t = h[(size_t)k];
    for (int e = 0; e < 3; e++) {
      const int nb = t.nb[e], a = t.v[(e + 1) % 3], b = t.v[(e + 2) % 3];
      int en = 0;
      if (nb > 0 && nb <= nt) {
        const TriRec &o = h[(size_t)nb];
        for (int f = 0; f < 3; f++) {
          const int c = o.v[(f + 1) % 3], d = o.v[(f + 2) % 3];
          if ((c == a && d == b) || (c == b && d == a)) en = f;
        }
      }
      adjt[3 * (k - 1) + 1 + e] = nb > 0 ? 3 * nb + en : 0;
    }
  }
  return nt;
}
