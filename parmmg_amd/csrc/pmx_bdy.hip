// pmx_bdy.hip -- surface (MG_BDY) part of the transfer path on gfx950.
//
// One thread per boundary vertex runs PMMG_locatePointBdy (reference
// src/locate_pmmg.c:587-723) with its shadow-wedge / shadow-cone tests
// (:209-334) and the PMMG_interp{3,2}bar / PMMG_copyMetrics dispatch of
// src/interpmesh_pmmg.c:550-599.
//
// Device semantics (documented in DESIGN.md): each query starts from the hint
// triangle instead of the previous query's result, and sees the old-mesh point
// flags in the state PMMG_precompute_nodeTrias leaves them (number of incident
// trias), with mesh->base = query ordinal + 1.  The flags a query writes
// (visited trias, wedge/cone marks) are kept in thread-private lists.
//
// Every kernel that walks the surface lives here, the sequential mode's
// replay (k_seq_resolve) included; the fans the walks read are built in
// pmx_fans.hip, the sequential modes are driven from pmx_seq.hip.
#include "pmx_device.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"
#include <algorithm>
#include <cmath>

#define UNSET (-1)

__device__ __constant__ int NXT2d[6] = {1, 2, 0, 1, 2, 0};

// thread-private query state: visited trias + point-flag overrides
template <int CAP> struct RegState {
  int vis[CAP];
  int ovp[CAP], ovf[CAP];
  int nv = 0, no = 0;
  bool over = false;
  __device__ void init(int *, int) {}
  __device__ int &V(int i) { return vis[i]; }
  __device__ int &OP(int i) { return ovp[i]; }
  __device__ int &OF(int i) { return ovf[i]; }
  static constexpr int cap() { return CAP; }
};
struct GlobState {
  int *vis, *ovp, *ovf;
  int nv = 0, no = 0, capv = 0;
  bool over = false;
  __device__ void init(int *ws, int cap) {
    vis = ws; ovp = ws + cap; ovf = ws + 2 * cap; capv = cap;
  }
  __device__ int &V(int i) { return vis[i]; }
  __device__ int &OP(int i) { return ovp[i]; }
  __device__ int &OF(int i) { return ovf[i]; }
};
// GlobState with hashed lists (the sequential mode's overflow pass: walks
// from the predecessors' trias run hundreds of steps, and the linear lists
// make each of them quadratic -- C3: 82-96 ms, a few walks long).  Open
// addressing in per-thread tables tagged with the walk's generation (its
// overflow-list position + 1; the caller zeroes the tables before the pass):
// the same set and map as the lists
struct GlobHashState {
  int2 *vt;                      // visited trias: (tria, gen)
  int4 *ft;                      // point flags: (point, gen, flag, -)
  int mask = 0, gen = 0, nv = 0, no = 0, capv = 0;
  bool over = false;
};
__device__ __forceinline__ unsigned ghs_hash(int x) { return (unsigned)x * 2654435761u; }
__device__ bool visited(GlobHashState &s, int t) {
  for (unsigned h = ghs_hash(t) & s.mask;; h = (h + 1) & s.mask) {
    const int2 e = s.vt[h];
    if (e.y != s.gen) return false;
    if (e.x == t) return true;
  }
}
__device__ void mark_visited(GlobHashState &s, int t) {
  unsigned h = ghs_hash(t) & s.mask;
  for (;; h = (h + 1) & s.mask) {
    const int2 e = s.vt[h];
    if (e.y != s.gen) break;
    if (e.x == t) return;
  }
  if (s.nv >= s.capv) { s.over = true; return; }
  s.vt[h] = make_int2(t, s.gen);
  s.nv++;
}
__device__ int get_flag(GlobHashState &s, int p, int cnt) {
  for (unsigned h = ghs_hash(p) & s.mask;; h = (h + 1) & s.mask) {
    const int4 e = s.ft[h];
    if (e.y != s.gen) return cnt;
    if (e.x == p) return e.z;
  }
}
__device__ void set_flag(GlobHashState &s, int p, int f) {
  unsigned h = ghs_hash(p) & s.mask;
  for (;; h = (h + 1) & s.mask) {
    const int4 e = s.ft[h];
    if (e.y != s.gen) break;
    if (e.x == p) { s.ft[h].z = f; return; }
  }
  if (s.no >= s.capv) { s.over = true; return; }
  s.ft[h] = make_int4(p, s.gen, f, 0);
  s.no++;
}

// the reference's own state, for the sequential replay (one lane): tria
// flags tf[] compared with mesh->base, point flags pf[] kept across queries
// (PF_INIT, pmx_kernels.h: still the incident-tria count
// PMMG_precompute_nodeTrias left)
struct SeqState {
  int *tf, *pf;
  int base;
  bool over = false;
};
// (agent-scope accesses: the replaying lane reads back what it wrote in
// earlier queries, never a stale L1 line)
__device__ __forceinline__ int ld_flag(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_flag(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool visited(SeqState &s, int t) { return ld_flag(s.tf + t) == s.base; }
__device__ __forceinline__ void mark_visited(SeqState &s, int t) { st_flag(s.tf + t, s.base); }
__device__ __forceinline__ int get_flag(SeqState &s, int p, int cnt) {
  const int f = ld_flag(s.pf + p);
  return f == PF_INIT ? cnt : f;
}
__device__ __forceinline__ void set_flag(SeqState &s, int p, int f) { st_flag(s.pf + p, f); }

template <class St> __device__ __forceinline__ int st_cap(const St &s);
template <int C> __device__ __forceinline__ int st_cap(const RegState<C> &) { return C; }
template <> __device__ __forceinline__ int st_cap(const GlobState &s) { return s.capv; }

// RegState: every access at a compile-time index (unrolled, predicated), so
// the lists live in VGPRs; a runtime index would put them in scratch and make
// each visited / flag lookup a dependent memory round trip (r01: the surface
// walk was latency-bound on exactly that)
template <int C> __device__ __forceinline__ bool visited(RegState<C> &s, int t) {
  bool h = false;
#pragma unroll
  for (int i = 0; i < C; i++) h |= (i < s.nv) & (s.vis[i] == t);
  return h;
}
template <int C> __device__ __forceinline__ void mark_visited(RegState<C> &s, int t) {
  if (visited(s, t)) return;
  if (s.nv >= C) { s.over = true; return; }
#pragma unroll
  for (int i = 0; i < C; i++)
    if (i == s.nv) s.vis[i] = t;
  s.nv++;
}
// flag of point p: the query's own override, else the incident-tria count
// PMMG_precompute_nodeTrias leaves (cnt, from the caller's fan record)
template <int C> __device__ __forceinline__ int get_flag(RegState<C> &s, int p, int cnt) {
  bool hit = false;
  int f = 0;
#pragma unroll
  for (int i = 0; i < C; i++) {
    const bool m = (i < s.no) & (s.ovp[i] == p);
    f = m ? s.ovf[i] : f;
    hit |= m;
  }
  return hit ? f : cnt;
}
template <int C> __device__ __forceinline__ void set_flag(RegState<C> &s, int p, int f) {
  bool upd = false;
#pragma unroll
  for (int i = 0; i < C; i++) {
    const bool m = (i < s.no) & (s.ovp[i] == p);
    s.ovf[i] = m ? f : s.ovf[i];
    upd |= m;
  }
  if (upd) return;
  if (s.no >= C) { s.over = true; return; }
#pragma unroll
  for (int i = 0; i < C; i++) {
    s.ovp[i] = (i == s.no) ? p : s.ovp[i];
    s.ovf[i] = (i == s.no) ? f : s.ovf[i];
  }
  s.no++;
}

template <class St> __device__ bool visited(St &s, int t) {
  for (int i = 0; i < s.nv; i++)
    if (s.V(i) == t) return true;
  return false;
}
template <class St> __device__ void mark_visited(St &s, int t) {
  if (visited(s, t)) return;
  if (s.nv >= st_cap(s)) { s.over = true; return; }
  s.V(s.nv++) = t;
}
template <class St> __device__ int get_flag(St &s, int p, int cnt) {
  for (int i = s.no - 1; i >= 0; i--)
    if (s.OP(i) == p) return s.OF(i);
  return cnt;
}
template <class St> __device__ void set_flag(St &s, int p, int f) {
  for (int i = 0; i < s.no; i++)
    if (s.OP(i) == p) { s.OF(i) = f; return; }
  if (s.no >= st_cap(s)) { s.over = true; return; }
  s.OP(s.no) = p;
  s.OF(s.no) = f;
  s.no++;
}

// PMMG_quickarea (src/barycoord_pmmg.c:41-59)
__device__ __forceinline__ double qarea(D3 a, D3 b, D3 c, D3 n) {
  double abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
  double acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
  double a0 = aby * acz - abz * acy, a1 = abz * acx - abx * acz, a2 = abx * acy - aby * acx;
  return a0 * n.x + a1 * n.y + a2 * n.z;
}

struct Bary { double val[4]; int idx[4]; };

// PMMG_barycoord2d_compute + sort + isInside (src/barycoord_pmmg.c:191-223,
// :274-284) on the geometry P (area) of a tria with the unit normal n;
// returns the signed normal distance h in b.val[3]
__device__ __forceinline__ bool tria_eval_pre(const D3 P[3], D3 n, double area, D3 p, Bary &b) {
  const D3 c = P[0];
  double h = 0.0;
  h += (p.x - c.x) * n.x;
  h += (p.y - c.y) * n.y;
  h += (p.z - c.z) * n.z;
  D3 q{p.x - h * n.x, p.y - h * n.y, p.z - h * n.z};
  b.val[0] = qarea(q, P[1], P[2], n) / area;
  b.val[1] = qarea(q, P[2], P[0], n) / area;
  b.val[2] = qarea(q, P[0], P[1], n) / area;
  b.idx[0] = 0; b.idx[1] = 1; b.idx[2] = 2;
  b.val[3] = h; b.idx[3] = 3;
  sort3(b.val, b.idx);
  return b.val[0] > -PMX_EPS;
}

__device__ bool tria_eval(const BdyArgs &A, int g, int kn, D3 p, Bary &b) {
  const TriRec t = A.tris[g];
  const Pt4 nn = A.trn[kn];
  const D3 P[3] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2])};
  return tria_eval_pre(P, D3{nn.x, nn.y, nn.z}, A.trn[g].w, p, b);
}

__device__ __forceinline__ double norm3(double a, double b, double c) {
  double r = 0.0;
  r += a * a;
  r += b * b;
  r += c * c;
  return sqrt(r);
}

// centroid distance of a tria (closest tracking, src/locate_pmmg.c:398-416)
__device__ __forceinline__ double centroid_dist_pre(const D3 P[3], D3 p) {
  double d0 = p.x, d1 = p.y, d2 = p.z;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    d0 -= P[j].x / 3.0;
    d1 -= P[j].y / 3.0;
    d2 -= P[j].z / 3.0;
  }
  return norm3(d0, d1, d2);
}
__device__ __forceinline__ double centroid_dist(const BdyArgs &A, int g, D3 p) {
  const TriRec t = A.tris[g];
  const D3 P[3] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2])};
  return centroid_dist_pre(P, p);
}

// PMMG_locatePointInTria (src/locate_pmmg.c:385-423), geometry g, normal kn:
// the tria, its normal and its 3 vertices are gathered once; the evaluation,
// the centroid distance and PMMG_locateChkDistTria (:347-366, the same h as
// the evaluation: vertex 0 of g against the normal of kn) share them
template <class St>
__device__ __forceinline__ bool in_tria(const BdyArgs &A, St &s, int g, int kn, D3 p, Bary &b, double &cdist,
                        int &ctria) {
  mark_visited(s, g);
  const TriRec t = A.tris[g];
  const Pt4 nn = A.trn[kn];
  const double area = A.trn[g].w;
  const D3 P[3] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2])};
  const bool found = tria_eval_pre(P, D3{nn.x, nn.y, nn.z}, area, p, b);
  const double nrm = centroid_dist_pre(P, p);
  if (nrm < cdist) { cdist = nrm; ctria = kn; }
  if (fabs(b.val[3]) > A.hausd) return false;
  return found;
}

// PMMG_locatePointInWedge (src/locate_pmmg.c:286-334)
template <class St>
__device__ int in_wedge(const BdyArgs &A, St &s, int k, int l, D3 p, int base, Bary &b) {
  int i0 = NXT2d[l], i1 = NXT2d[l + 1];   // inxt2[l], iprv2[l]
  TriRec t = A.tris[k];
  int q0 = t.v[i0], q1 = t.v[i1];
  D3 c0 = ld3(A.xyz, q0), c1 = ld3(A.xyz, q1);
  double pv[3] = {p.x - c0.x, p.y - c0.y, p.z - c0.z};
  double a[3] = {c1.x - c0.x, c1.y - c0.y, c1.z - c0.z};
  double n2 = 0.0, alpha = 0.0, dist = 0.0;
  for (int d = 0; d < 3; d++) n2 += a[d] * a[d];
  for (int d = 0; d < 3; d++) alpha += a[d] * pv[d];
  for (int d = 0; d < 3; d++) pv[d] -= (alpha / n2) * a[d];
  for (int d = 0; d < 3; d++) dist += pv[d] * pv[d];
  dist = sqrt(dist);
  if (dist > A.hausd) return UNSET;
  if (alpha < 0.0) { set_flag(s, q1, base); return i0; }
  if (alpha > n2) { set_flag(s, q0, base); return i1; }
  b.idx[0] = 0; b.idx[1] = 1; b.idx[2] = 2;
  b.val[l] = 0.0;
  b.val[i0] = 1.0 - alpha / n2;
  b.val[i1] = alpha / n2;
  return 4;
}

// PMMG_locatePointInCone (src/locate_pmmg.c:209-270)
template <class St>
__device__ bool in_cone(const BdyArgs &A, St &s, int k, int iloc, D3 p, int base) {
  int ip = A.tris[k].v[iloc];
  D3 c0 = ld3(A.xyz, ip);
  set_flag(s, ip, base);
  double pv[3] = {p.x - c0.x, p.y - c0.y, p.z - c0.z};
  double dist = 0.0;
  for (int d = 0; d < 3; d++) dist += pv[d] * pv[d];
  dist = sqrt(dist);
  const int2 fan = A.ntrange[3 * k + iloc];
  for (int f = fan.x; f < fan.y; f++) {
    const int g = A.ntlist[f];
    TriRec t = A.tris[g];
    for (int j = 0; j < 3; j++) {
      int jp = t.v[j];
      if (jp == ip) continue;
      const int2 r = A.ntrange[3 * g + j];
      if (get_flag(s, jp, r.y - r.x) == ip) continue;
      set_flag(s, jp, ip);
      D3 cj = ld3(A.xyz, jp);
      double a[3] = {cj.x - c0.x, cj.y - c0.y, cj.z - c0.z};
      if (dist > A.hausd) return false;
      double alpha = 0.0;
      for (int d = 0; d < 3; d++) alpha += a[d] * pv[d];
      if (alpha > 0.0) return false;
    }
  }
  return true;
}

// ---- interpolation on a boundary triangle --------------------------------

// keep (may be null): where the barycentrics, in the tria's vertex order, are
// kept for pmx_interp_more -- the walk's barycoord array as PMMG_barycoord_get
// orders it is not a function of (tria, point) alone: a shadow-wedge hit
// rewrites it, the exhaustive not-found branch evaluates it on another tria's
// geometry
__device__ void interp_tria(const BdyArgs &A, int k, const Bary &b, int edge, int vtx,
                            double *out, unsigned &wm, Pt4 *keep = nullptr) {
  TriRec t = A.tris[k];
  int v[3] = {t.v[0], t.v[1], t.v[2]};
  double phi[3];
  // PMMG_barycoord_get(phi, barycoord, 3)
  for (int i = 0; i < 3; i++) {
    int id = b.idx[i];
    double val = b.val[i];
    if (id == 0) phi[0] = val;
    if (id == 1) phi[1] = val;
    if (id == 2) phi[2] = val;
  }
  if (keep) *keep = Pt4{phi[0], phi[1], phi[2], 0.0};
  const SolDesc &sd = A.sd;
  for (int s = 0; s < sd.nsol; ++s) {
    if (s == sd.imet && sd.metric_const) continue;
    const int sz = sd.size[s], off = sd.off[s];
    const bool met = (s == sd.imet);
    if (met && vtx != UNSET) {                       // PMMG_copyMetrics
      int src = v[0];
      if (vtx == 1) src = v[1];
      if (vtx == 2) src = v[2];
      for (int j = 0; j < sz; j++) out[off + j] = A.sol[(int64_t)src * sd.S + off + j];
      wm |= 1u << s;
    } else if (met && edge != UNSET) {               // PMMG_interp2bar_{iso,ani}
      int i0 = NXT2d[edge], i1 = NXT2d[edge + 1];
      int va = v[0], vb = v[0];
      double pa = phi[0], pb = phi[0];
      if (i0 == 1) { va = v[1]; pa = phi[1]; }
      if (i0 == 2) { va = v[2]; pa = phi[2]; }
      if (i1 == 1) { vb = v[1]; pb = phi[1]; }
      if (i1 == 2) { vb = v[2]; pb = phi[2]; }
      if (sz == 1) {
        out[off] = pa * A.sol[(int64_t)va * sd.S + off] + pb * A.sol[(int64_t)vb * sd.S + off];
        wm |= 1u << s;
      } else {
        double m0[6], m1[6], mi0[6], mi1[6], mint[6], r[6];
        for (int j = 0; j < 6; j++) {
          m0[j] = A.sol[(int64_t)va * sd.S + off + j];
          m1[j] = A.sol[(int64_t)vb * sd.S + off + j];
        }
        if (!invmat(m0, mi0)) continue;
        if (!invmat(m1, mi1)) continue;
        for (int j = 0; j < 6; j++) mint[j] = pa * mi0[j] + pb * mi1[j];
        if (!invmat(mint, r)) continue;
        for (int j = 0; j < 6; j++) out[off + j] = r[j];
        wm |= 1u << s;
      }
    } else if (sz == 6) {                             // PMMG_interp3bar_ani
      double mi[3][6], mint[6], r[6];
      bool okk = true;
      // unrolled (static indices keep mi in VGPRs); && stops at the first
      // failed inversion like the reference loop
#pragma unroll
      for (int i = 0; i < 3; i++) {
        double m[6];
#pragma unroll
        for (int j = 0; j < 6; j++) m[j] = A.sol[(int64_t)v[i] * sd.S + off + j];
        okk = okk && invmat(m, mi[i]);
      }
      if (!okk) continue;
      for (int j = 0; j < 6; j++) mint[j] = phi[0] * mi[0][j] + phi[1] * mi[1][j] + phi[2] * mi[2][j];
      if (!invmat(mint, r)) continue;
      for (int j = 0; j < 6; j++) out[off + j] = r[j];
      wm |= 1u << s;
    } else {                                          // PMMG_interp3bar_iso
      for (int j = 0; j < sz; j++) {
        double acc = 0.0;
        for (int i = 0; i < 3; i++) acc += phi[i] * A.sol[(int64_t)v[i] * sd.S + off + j];
        out[off + j] = acc;
      }
      wm |= 1u << s;
    }
  }
}

// ---- the walk ----------------------------------------------------------------

// returns 1 found, 2 stuck (needs exhaustive), 3 private-state overflow
template <class St>
__device__ int walk_bdy(const BdyArgs &A, St &s, D3 p, int start, int base, int &k, Bary &b,
                        int &edge, int &vtx, int &step, bool &wedged) {
  wedged = false;
  double cdist = 1.0e10;
  int ctria = 0;
  k = start;
  step = 0;
  edge = UNSET;
  vtx = UNSET;
  bool stuck = false;
  while (step <= A.nt && !stuck) {
    step++;
    TriRec t = A.tris[k];
    if (t.v[0] <= 0) { stuck = true; break; }
    if (in_tria(A, s, k, k, p, b, cdist, ctria)) {
      if (b.val[0] < PMX_EPS) {                        // PMMG_barycoord_isBorder
        if (b.val[1] < PMX_EPS) vtx = b.idx[2];
        else edge = b.idx[0];
      }
      return s.over ? 3 : 1;
    }
    if (s.over) return 3;
    int j;
    for (j = 0; j < 3; j++) {
      int i = b.idx[j];
      int nb = t.nb[0];
      if (i == 1) nb = t.nb[1];
      if (i == 2) nb = t.nb[2];
      if (!nb) continue;
      if (visited(s, nb)) {
        wedged = true;
        int il = in_wedge(A, s, k, i, p, base, b);
        if (s.over) return 3;
        if (il == UNSET) continue;
        if (il == 4) { edge = i; return 1; }
        bool c = in_cone(A, s, k, il, p, base);
        if (s.over) return 3;
        if (c) { vtx = il; return 1; }
        continue;
      }
      k = nb;
      break;
    }
    if (j == 3) stuck = true;
  }
  return 2;
}

// position of point i in the surface list (ascending: the compaction keeps
// the input order); for the finishers that know the point only (overflow
// pass, exhaustive scan, sequential replay -- a few points of a step)
__device__ int64_t bdy_slot(const BdyArgs &A, int64_t i) {
  int64_t lo = 0, hi = *A.nlist_dev;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A.list[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// slot: the point's position in the surface list (< 0: looked up)
__device__ void finish_bdy(const BdyArgs &A, int64_t i, int k, const Bary &b, int edge, int vtx,
                           int status, int step, int64_t slot = -1) {
  A.elem[i] = k;
  A.status[i] = status;
  A.steps[i] = step;
  A.edge[i] = edge;
  A.vertex[i] = vtx;
  if (slot < 0) slot = bdy_slot(A, i);
  // (only the list's own entry: a point that is not in the surface list keeps nothing)
  const bool mine = slot < *A.nlist_dev && slot < A.nlist && A.list[slot] == i;
  unsigned wm = 0;
  interp_tria(A, k, b, edge, vtx, A.out + i * A.sd.S, wm, mine ? A.bphi + slot : nullptr);
  A.wmask[i] = (uint8_t)(A.wmask[i] | wm);
}

__device__ int tria_hint(const BdyArgs &A, D3 p);

// PM (PMX_RUN_POINTMAP): the start tria is A.grid's, per list entry
template <int CAP, bool PM = false>
__global__ __launch_bounds__(256) void k_locate_bdy(BdyArgs A) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned s_cnt = 0, s_sum = 0, s_max = 0, s_min = 0xffffffffu;
  if (j < *A.nlist_dev) {
    const int64_t i = A.list[j];
    const D3 p = ld3(A.q, (int)i);
    int start;
    if constexpr (PM) start = A.grid[j];
    else start = A.seq_start ? A.seq_start[i] : tria_hint(A, p);
    const int base = A.seq_base ? A.seq_base[i] : (int)(i + 1);
    A.start[i] = start;
    RegState<CAP> s;
    Bary b;
    int k, edge, vtx, step;
    bool wedged;
    int r = walk_bdy(A, s, p, start, base, k, b, edge, vtx, step, wedged);
    if (A.seq_w) A.seq_w[i] = wedged ? 1 : 0;
    if (r == 1) {
      finish_bdy(A, i, k, b, edge, vtx, 1, step, j);
      s_cnt = 1; s_sum = (unsigned)step; s_max = (unsigned)step; s_min = (unsigned)step;
    } else if (r == 2) {
      unsigned slot = atomicAdd(A.stuck_count, 1u);
      A.stuck_list[slot] = (int)i;
      A.steps[i] = -step;
    } else {
      unsigned slot = atomicAdd(A.ovf_count, 1u);
      A.ovf_list[slot] = (int)i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s_cnt += __shfl_xor(s_cnt, o, 64);
    s_sum += __shfl_xor(s_sum, o, 64);
    unsigned a = __shfl_xor(s_max, o, 64), b = __shfl_xor(s_min, o, 64);
    s_max = a > s_max ? a : s_max;
    s_min = b < s_min ? b : s_min;
  }
  if ((threadIdx.x & 63) == 0) A.wstats[j / 64] = make_uint4(s_cnt, s_sum, s_max, s_min);
}

// overflow pass: same walk with large lists in a global workspace
__global__ __launch_bounds__(64) void k_locate_bdy_ovf(BdyArgs A, int *ws, int cap) {
  const unsigned n = *A.ovf_count;
  const unsigned nthr = gridDim.x * blockDim.x;
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
  for (unsigned j = tid; j < n; j += nthr) {
    int64_t i = A.ovf_list[j];
    const D3 p = ld3(A.q, (int)i);
    GlobState s;
    s.init(ws + (size_t)tid * 3 * cap, cap);
    Bary b;
    int k, edge, vtx, step;
    bool wedged;
    int r = walk_bdy(A, s, p, A.start[i], A.seq_base ? A.seq_base[i] : (int)(i + 1), k, b, edge, vtx, step,
                     wedged);
    if (A.seq_w) A.seq_w[i] = wedged ? 1 : 0;
    if (r == 1) {
      finish_bdy(A, i, k, b, edge, vtx, 1, step);
    } else {
      unsigned slot = atomicAdd(A.stuck_count, 1u);
      A.stuck_list[slot] = (int)i;
      A.steps[i] = -step;
    }
  }
}

// the sequential mode's overflow pass, on hashed lists (workspace:
// GHS_WS_INTS ints per thread, zeroed by the caller)
__global__ __launch_bounds__(64) void k_locate_bdy_ovf_hash(BdyArgs A, int *ws) {
  const unsigned n = *A.ovf_count;
  const unsigned nthr = gridDim.x * blockDim.x;
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
  int *w = ws + (size_t)tid * GHS_WS_INTS;
  for (unsigned j = tid; j < n; j += nthr) {
    int64_t i = A.ovf_list[j];
    const D3 p = ld3(A.q, (int)i);
    GlobHashState s;
    s.vt = reinterpret_cast<int2 *>(w);
    s.ft = reinterpret_cast<int4 *>(w + 2 * GHS_SLOTS);
    s.mask = GHS_SLOTS - 1;
    s.capv = GHS_SLOTS / 2;
    s.gen = (int)j + 1;
    Bary b;
    int k, edge, vtx, step;
    bool wedged;
    int r = walk_bdy(A, s, p, A.start[i], A.seq_base ? A.seq_base[i] : (int)(i + 1), k, b, edge, vtx, step,
                     wedged);
    if (A.seq_w) A.seq_w[i] = wedged ? 1 : 0;
    if (r == 1) {
      finish_bdy(A, i, k, b, edge, vtx, 1, step);
    } else {
      unsigned slot = atomicAdd(A.stuck_count, 1u);
      A.stuck_list[slot] = (int)i;
      A.steps[i] = -step;
    }
  }
}

// Exhaustive surface search (PMMG_locatePoint_exhaustTria, :477-515):
// one workgroup per stuck point.  First containing tria in index order, else
// the closest tria by centroid distance (lowest index on ties) and the
// reference's re-evaluation with the last tria's geometry.
__global__ __launch_bounds__(256) void k_exh_bdy(BdyArgs A) {
  __shared__ int s_min;
  __shared__ double s_d[256];
  __shared__ int s_k[256];
  const unsigned n = *A.stuck_count;
  for (unsigned j = blockIdx.x; j < n; j += gridDim.x) {
    int64_t i = A.stuck_list[j];
    const D3 p = ld3(A.q, (int)i);
    if (threadIdx.x == 0) s_min = 0x7fffffff;
    __syncthreads();
    RegState<1> dummy;
    for (int64_t t = 1 + threadIdx.x; t <= A.nt; t += blockDim.x) {
      if (A.tris[t].v[0] <= 0) continue;
      Bary b;
      double cd = 1e300;
      int ct = 0;
      dummy.nv = 0;
      dummy.over = false;
      if (in_tria(A, dummy, (int)t, (int)t, p, b, cd, ct)) {
        atomicMin(&s_min, (int)t);
        break;   // later t of this thread are larger
      }
    }
    __syncthreads();
    int kf = s_min;
    if (kf != 0x7fffffff) {
      if (threadIdx.x == 0) {
        Bary b;
        tria_eval(A, kf, kf, p, b);
        finish_bdy(A, i, kf, b, UNSET, UNSET, -1, A.steps[i] - 1);
      }
    } else {
      double best = 1.0e10;
      int bk = 0x7fffffff;
      for (int64_t t = 1 + threadIdx.x; t <= A.nt; t += blockDim.x) {
        if (A.tris[t].v[0] <= 0) continue;
        double d = centroid_dist(A, (int)t, p);
        if (d < best || (d == best && (int)t < bk)) { best = d; bk = (int)t; }
      }
      s_d[threadIdx.x] = best;
      s_k[threadIdx.x] = bk;
      __syncthreads();
      for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
          double d2 = s_d[threadIdx.x + o];
          int k2 = s_k[threadIdx.x + o];
          if (d2 < s_d[threadIdx.x] || (d2 == s_d[threadIdx.x] && k2 < s_k[threadIdx.x])) {
            s_d[threadIdx.x] = d2;
            s_k[threadIdx.x] = k2;
          }
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        int ct = s_k[0];
        Bary b;
        RegState<1> d1;
        double cd = 1e300;
        int cc = 0;
        if (!in_tria(A, d1, (int)A.nt, ct, p, b, cd, cc)) {
          // PMMG_barycoord2d_getClosest (src/barycoord_pmmg.c:324-357)
          TriRec t = A.tris[ct];
          double bd = 0.0;
          int it = 0;
          for (int l = 0; l < 3; l++) {
            D3 c = ld3(A.xyz, t.v[l]);
            double d = norm3(p.x - c.x, p.y - c.y, p.z - c.z);
            if (l == 0 || d < bd) { bd = d; it = l; }
          }
          for (int l = 0; l < 3; l++) { b.idx[l] = l; b.val[l] = (l == it) ? 1.0 : 0.0; }
        }
        finish_bdy(A, i, ct, b, UNSET, UNSET, 0, A.steps[i] - 1);
      }
    }
    __syncthreads();
  }
}

// tria hint grid: cell -> largest tria index whose centroid falls in it
// (deterministic: the surface semantics depend on the start triangle)
__device__ __forceinline__ void tria_hint_one(const TriRec *tris, const double *xyz, int64_t k, int *grid,
                                              const GridDesc &g) {
  TriRec t = tris[k];
  if (t.v[0] <= 0) return;
  D3 a = ld3(xyz, t.v[0]), b = ld3(xyz, t.v[1]), c = ld3(xyz, t.v[2]);
  D3 m{(a.x + b.x + c.x) / 3.0, (a.y + b.y + c.y) / 3.0, (a.z + b.z + c.z) / 3.0};
  int cx = (int)fmin(fmax((m.x - g.lo[0]) * g.inv[0], 0.0), (double)(g.dim[0] - 1));
  int cy = (int)fmin(fmax((m.y - g.lo[1]) * g.inv[1], 0.0), (double)(g.dim[1] - 1));
  int cz = (int)fmin(fmax((m.z - g.lo[2]) * g.inv[2], 0.0), (double)(g.dim[2] - 1));
  atomicMax(&grid[(int64_t)cx + (int64_t)g.dim[0] * ((int64_t)cy + (int64_t)g.dim[1] * cz)], (int)k);
}
__global__ __launch_bounds__(256) void k_tria_hint_build(const TriRec *tris, const double *xyz,
                                                         int64_t nt, int *grid, GridDesc g) {
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nt;
       k += (int64_t)gridDim.x * blockDim.x)
    tria_hint_one(tris, xyz, k, grid, g);
}

__device__ int tria_hint(const BdyArgs &A, D3 p) {
  const GridDesc &g = A.g;
  int c[3];
  c[0] = (int)fmin(fmax((p.x - g.lo[0]) * g.inv[0], 0.0), (double)(g.dim[0] - 1));
  c[1] = (int)fmin(fmax((p.y - g.lo[1]) * g.inv[1], 0.0), (double)(g.dim[1] - 1));
  c[2] = (int)fmin(fmax((p.z - g.lo[2]) * g.inv[2], 0.0), (double)(g.dim[2] - 1));
  int k = A.grid[(int64_t)c[0] + (int64_t)g.dim[0] * ((int64_t)c[1] + (int64_t)g.dim[1] * c[2])];
  if (k) return k;
  for (int r = 1; r <= 4; r++)
    for (int dz = -r; dz <= r; dz++)
      for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++) {
          if (max(abs(dx), max(abs(dy), abs(dz))) != r) continue;
          int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
          if (x < 0 || y < 0 || z < 0 || x >= g.dim[0] || y >= g.dim[1] || z >= g.dim[2]) continue;
          int kk = A.grid[(int64_t)x + (int64_t)g.dim[0] * ((int64_t)y + (int64_t)g.dim[1] * z)];
          if (kk) return kk;
        }
  return 1;
}

// surface walks are short (1.5 steps on C2): 16 private slots, the rare longer
// walk is redone by k_locate_bdy_ovf with a global workspace (r03: with 8
// slots the overflow pass, one long serial walk per thread, was the C2 surface
// path's tail: surface path 0.287 -> 0.217 ms, step 0.336 -> 0.328 ms with 16;
// C3 within 0.1 %; profiles/r03_c{2,3}_sweep_bdy_cap.log)
#define BDY_CAP 16
#define OVF_CAP 2048

// the coarser tria hint grid over the background bbox: cells of about 8
// boundary trias.  The grid is 3-D but only its surface cells are used, so it
// is zeroed and rebuilt every step for mostly empty cells; at 2 trias per
// cell it was a 66-MB memset per C3 step beside the volume walk (r02 profile),
// at 8 it is 8.4 MB (surface walks of ~1 more step, latency on the side stream)
bool pmx_ctx::size_tria_grid() {
  double ext[3];
  int64_t cells = 1;
  for (int ax = 0; ax < 3; ax++) ext[ax] = std::max(bbhi[ax] - bblo[ax], 1e-300);
  const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]);
  const double h = std::sqrt(area / std::max(1.0, (double)nt / 8.0));
  for (int ax = 0; ax < 3; ax++) {
    // 1e-9 slack: libm cbrt/sqrt are not correctly rounded and a cell count
    // of exactly n must not become n+1 (misaligned with a lattice-like mesh)
    int d = (int)std::ceil(ext[ax] / h * (1.0 - 1e-9));
    d = std::max(1, std::min(d, 1024));
    tgd.dim[ax] = d;
    tgd.lo[ax] = bblo[ax];
    tgd.inv[ax] = (double)d / ext[ax];
    cells *= d;
  }
  tcells = nt > 0 ? cells : 0;
  return !tcells || pmx_call{this, "tria hint grid"}.grow(d_tgrid, (size_t)cells);
}

// the surface kernels' arguments for the step's points (tria hint grid tgd)
BdyArgs bdy_args(pmx_ctx *c, const VolArgs &a, bool pointmap) {
  BdyArgs B{};
  B.xyz = c->d_xyz.p; B.tris = c->d_tris.p; B.trn = c->d_trn.p; B.ntrange = c->d_ntrange.p; B.ntlist = c->d_ntlist.p;
  B.sol = c->d_sol.p; B.sd = a.sd; B.q = c->d_qxyz.p; B.kind = c->d_kind.p; B.nq = c->nq; B.nt = c->nt;
  B.hausd = c->hausd; B.grid = c->d_tgrid.p; B.g = c->tgd;
  B.out = c->d_out.p; B.wmask = c->d_wmask.p; B.elem = c->d_elem.p; B.status = c->d_status.p;
  B.steps = c->d_steps.p; B.start = c->d_start.p; B.edge = c->d_edge.p; B.vertex = c->d_vertex.p;
  B.bphi = c->d_bphi.p;
  B.stuck_list = c->d_blist.p; B.stuck_count = c->d_counts.p + 1;
  B.ovf_list = c->d_olist.p; B.ovf_count = c->d_counts.p + 2;
  B.list = c->d_bdylist.p; B.nlist = c->nq_bdy_ub; B.nlist_dev = c->d_nsel.p + 1; B.wstats = c->d_bstat.p;
  if (pointmap) B.grid = a.grid + a.nq;      // the surface list's start trias (k_cls_write)
  return B;
}

// the walks, their private-list overflow pass and the exhaustive scan (pmx_kernels.h)
void launch_bdy_walks(const BdyArgs &B, int *ows, hipStream_t s, int ovf_threads, bool hashed, bool pointmap) {
  const int64_t nb = (B.nlist + 255) / 256;
  if (pointmap)
    hipLaunchKernelGGL((k_locate_bdy<BDY_CAP, true>), dim3((unsigned)nb), dim3(256), 0, s, B);
  else
    hipLaunchKernelGGL(k_locate_bdy<BDY_CAP>, dim3((unsigned)nb), dim3(256), 0, s, B);
  if (hashed)
    hipLaunchKernelGGL(k_locate_bdy_ovf_hash, dim3(ovf_threads / 64), dim3(64), 0, s, B, ows);
  else
    hipLaunchKernelGGL(k_locate_bdy_ovf, dim3(ovf_threads / 64), dim3(64), 0, s, B, ows, OVF_CAP);
  launch_exh_bdy(B, 256, s);
}

bool pmx_ctx::launch_bdy(const VolArgs &a, hipStream_t s, bool pointmap) {
  const pmx_call C{this, "surface locate", s};
  if (nt < 1) return C.fail("surface points present but the background has no boundary trias");
  // the overflow workspace: allocated once (the sequential mode grows it for its own pass)
  if (!C.grow(d_blist, (size_t)nq) || !C.grow(d_olist, (size_t)nq) ||
      !C.grow(d_bphi, (size_t)std::max<int64_t>(nq_bdy_ub, 1)) ||
      (!d_ows.p && !C.grow(d_ows, (size_t)OVF_THREADS * 3 * OVF_CAP)))
    return false;
  // tria hint grid: sized and allocated with the background
  // (pmx_ctx::size_tria_grid), zeroed and built at the head of the surface
  // path (off the main stream); none with point-map starts
  if (!pointmap) {
    if (!C.hip(hipMemsetAsync(d_tgrid.p, 0, sizeof(int) * (size_t)tcells, s), "tria hint grid memset")) return false;
    int64_t nb = (nt + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_tria_hint_build, dim3((unsigned)std::max<int64_t>(nb, 1)), dim3(256), 0, s,
                       d_tris.p, d_xyz.p, nt, d_tgrid.p, tgd);
    tgrid_built = true;
  }
  launch_bdy_walks(bdy_args(this, a, pointmap), d_ows.p, s, OVF_THREADS, false, pointmap);
  return C.hip(hipGetLastError(), "launch");
}

// the replay, one lane, in visit order over the candidate positions (cand,
// sorted) and the successor of every replayed query; ctl = {next position,
// its start (-1: the tria of the previous point, after a stuck walk the host
// resolved), state (0 done, 1 stuck), the point}.  (r06 first version: the
// wave scanned all positions, 64 at a time.)
__global__ __launch_bounds__(64) void k_seq_resolve(BdyArgs A, const int *__restrict__ seq,
                                                    const int *__restrict__ nseq_p, const int *__restrict__ sstart,
                                                    const uint8_t *__restrict__ sw, const int *__restrict__ sbase,
                                                    int *tf, int *pf, int *ctl, int *stk_list,
                                                    unsigned *stk_count, unsigned *nreplay,
                                                    const int *__restrict__ cand, const int *__restrict__ ncand) {
  if (threadIdx.x != 0) return;
  const int nseq = *nseq_p;
  int j = ctl[0];
  int prev = ctl[1];
  if (j >= nseq) return;
  bool dirty = prev < 0;
  if (prev < 0) prev = A.elem[seq[j - 1]];
  const int nc = *ncand;
  int lo = 0, hi = nc;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cand[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  int pos = lo;
  unsigned replays = 0;
  while (j < nseq) {
    if (!dirty) {
      while (pos < nc && cand[pos] < j) pos++;
      if (pos >= nc) break;
      const int c = cand[pos];
      if (c > j) {
        prev = A.elem[seq[c - 1]];
        j = c;
      }
    }
    const int i = seq[j];
    if (!sw[i] && sstart[i] == prev) {
      prev = A.elem[i];
      dirty = false;
      j++;
      continue;
    }
    const D3 p = ld3(A.q, i);
    SeqState st{tf, pf, sbase[i]};
    Bary b;
    int k, edge, vtx, step;
    bool wedged;
    A.start[i] = prev;
    const int r = walk_bdy(A, st, p, prev, sbase[i], k, b, edge, vtx, step, wedged);
    replays++;
    if (r != 1) {
      A.steps[i] = -step;
      stk_list[0] = i;
      *stk_count = 1u;
      ctl[0] = j;
      ctl[2] = 1;
      ctl[3] = i;
      atomicAdd(nreplay, replays);
      return;
    }
    finish_bdy(A, i, k, b, edge, vtx, 1, step);
    prev = k;
    dirty = true;
    j++;
  }
  ctl[0] = nseq;
  ctl[2] = 0;
  atomicAdd(nreplay, replays);
}

void launch_seq_resolve(const BdyArgs &B, const SeqBdyArgs &q, hipStream_t s) {
  hipLaunchKernelGGL(k_seq_resolve, dim3(1), dim3(64), 0, s, B, q.seq, q.nseq, q.sstart, q.sw, q.sbase, q.tf, q.pf,
                     q.ctl, q.stk_list, q.stk_count, q.nreplay, q.cand, q.ncand);
}
void launch_exh_bdy(const BdyArgs &B, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_exh_bdy, dim3((unsigned)blocks), dim3(256), 0, s, B);
}
