// pmx_metric.h -- Mmg's per-tet quality and per-edge length in a metric
// (device only): what the quality pass (pmx_quality.hip), the edge-length
// statistics (pmx_lengths.hip) and the Metis graph's weights (pmx_graph.hip)
// all evaluate on a StatArgs view.
//
// tet_quality          <- MMG5_caltet_iso / MMG5_caltet33_ani, and
//                         MMG5_caltet_ani (metRidTyp = 1) past MMG5_moymet
// edge_len[_t], iso_edge_*, ani_edge_len <- MMG5_lenedg_iso / lenedg33_ani
// len_tet_ani, len_surf_ani <- MMG5_lenedg_ani / MMG5_lenSurfEdg[33]_ani with
//                         MMG5_buildridmet and MMG5_lenedgspl_ani
// len_iso_flat         <- MMG5_lenSurfEdg_iso on the flat size-6 array
//                         (reference src/quality_pmmg.c:466)
// pmx_log1p            <- glibc's log1p, bit for bit (the iso lengths)
// All restated from Mmg's public sources, unpinned.
//
// The library is built without relocatable device code: every translation
// unit that includes this header holds its own copy of what it uses, so the
// functions that are not __forceinline__ are static.
#pragma once
#include "pmx_kernels.h"

#define TAG_GEO 2
#define TAG_REQ 4
#define TAG_NOM 8
#define TAG_CRN 32
#define TAG_REF 1

// MMG5_caltet_iso (restated)
static __device__ double caltet_iso(D3 a, D3 b, D3 c, D3 d) {
  double abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
  double acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
  double adx = d.x - a.x, ady = d.y - a.y, adz = d.z - a.z;
  double v1 = acy * adz - acz * ady;
  double v2 = acz * adx - acx * adz;
  double v3 = acx * ady - acy * adx;
  double vol = abx * v1 + aby * v2 + abz * v3;
  if (vol <= 0.) return 0.0;
  double bcx = c.x - b.x, bcy = c.y - b.y, bcz = c.z - b.z;
  double bdx = d.x - b.x, bdy = d.y - b.y, bdz = d.z - b.z;
  double cdx = d.x - c.x, cdy = d.y - c.y, cdz = d.z - c.z;
  double rap = abx * abx + aby * aby + abz * abz;
  rap += acx * acx + acy * acy + acz * acz;
  rap += adx * adx + ady * ady + adz * adz;
  rap += bcx * bcx + bcy * bcy + bcz * bcz;
  rap += bdx * bdx + bdy * bdy + bdz * bdz;
  rap += cdx * cdx + cdy * cdy + cdz * cdz;
  if (rap < PMX_EPSD2) return 0.0;
  rap = rap * sqrt(rap);
  return vol / rap;
}

__device__ __forceinline__ double mlen2(const double *m, double x, double y, double z) {
  return m[0] * x * x + m[3] * y * y + m[5] * z * z + 2.0 * (m[1] * x * y + m[2] * x * z + m[4] * y * z);
}

// MMG5_caltet33_ani / MMG5_caltet_ani (restated) past their mean metric mm
static __device__ double caltet_ani_mm(D3 a, D3 b, D3 c, D3 d, const double mm[6]) {
  double abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
  double acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
  double adx = d.x - a.x, ady = d.y - a.y, adz = d.z - a.z;
  double vol = abx * (acy * adz - acz * ady) + aby * (acz * adx - acx * adz) + abz * (acx * ady - acy * adx);
  if (vol <= 0.) return 0.0;
  double det = mm[0] * (mm[3] * mm[5] - mm[4] * mm[4]) - mm[1] * (mm[1] * mm[5] - mm[2] * mm[4]) +
               mm[2] * (mm[1] * mm[4] - mm[2] * mm[3]);
  if (det < PMX_EPSD2) return 0.0;
  det = sqrt(det) * vol;
  double bcx = c.x - b.x, bcy = c.y - b.y, bcz = c.z - b.z;
  double bdx = d.x - b.x, bdy = d.y - b.y, bdz = d.z - b.z;
  double cdx = d.x - c.x, cdy = d.y - c.y, cdz = d.z - c.z;
  double rap = mlen2(mm, abx, aby, abz);
  rap += mlen2(mm, acx, acy, acz);
  rap += mlen2(mm, adx, ady, adz);
  rap += mlen2(mm, bcx, bcy, bcz);
  rap += mlen2(mm, bdx, bdy, bdz);
  rap += mlen2(mm, cdx, cdy, cdz);
  if (rap < PMX_EPSD2) return 0.0;
  double num = sqrt(rap) * rap;
  return det / num;
}

// MMG5_caltet33_ani: the plain mean of the 4 vertex metrics
static __device__ double caltet_ani(D3 a, D3 b, D3 c, D3 d, const double *ma, const double *mb,
                                    const double *mc, const double *md) {
  double mm[6];
  for (int i = 0; i < 6; i++) mm[i] = 0.25 * (ma[i] + mb[i] + mc[i] + md[i]);
  return caltet_ani_mm(a, b, c, d, mm);
}

// vertex v of the statistics' mesh (the background: dense xyz; the new mesh:
// the uploaded Pt4 points, shifted by the first point index)
__device__ __forceinline__ D3 sld3(const StatArgs &A, int v) {
  const double *r = A.xyz + (int64_t)A.xstride * (v - A.vbase);
  return D3{r[0], r[1], r[2]};
}
__device__ __forceinline__ const double *smet(const StatArgs &A, int v) {
  return A.sol + (int64_t)(v - A.vbase) * A.S + A.moff;
}
__device__ __forceinline__ unsigned stag(const StatArgs &A, int v) { return A.ptag[v - A.vbase]; }

// a vertex that is a non-singular ridge point: !(MG_SIN || MG_NOM) && MG_GEO
__device__ __forceinline__ bool ridge_pt(unsigned tg) {
  const bool sin = (tg & TAG_CRN) || (tg & TAG_REQ);
  return !(sin || (TAG_NOM & tg)) && (tg & TAG_GEO);
}
// all 4 vertices are non-singular ridge points: skipped by the length loop
// (reference src/quality_pmmg.c:509-517), counted by MMG3D_computeOutqua's nrid
__device__ __forceinline__ bool tet_4ridge(const StatArgs &A, const int v[4]) {
  if (!A.ptag) return false;
  bool all = true;
#pragma unroll
  for (int i = 0; i < 4; i++) all = all && ridge_pt(stag(A, v[i]));
  return all;
}

// MMG5_caltet_ani (metRidTyp = 1): MMG5_moymet's mean over the vertices that
// are not non-singular ridge points (their stored metric is Mmg's two-sided
// ridge metric), summed in vertex order and scaled by 1/n; none: quality 0
static __device__ double caltet_ani_rid(const StatArgs &A, const int v[4], D3 a, D3 b, D3 c, D3 d) {
  double mm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int n = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (A.rtag && ridge_pt(A.rtag[v[j] - A.vbase])) continue;
    n++;
    const double *m = smet(A, v[j]);
#pragma unroll
    for (int i = 0; i < 6; i++) mm[i] += m[i];
  }
  if (!n) return 0.0;
  const double dd = 1. / n;
#pragma unroll
  for (int i = 0; i < 6; i++) mm[i] = mm[i] * dd;
  return caltet_ani_mm(a, b, c, d, mm);
}

template <bool ANI>
static __device__ double tet_quality(const StatArgs &A, const int v[4]) {
  D3 a = sld3(A, v[0]), b = sld3(A, v[1]), c = sld3(A, v[2]), d = sld3(A, v[3]);
  if (ANI && A.ridmet) return caltet_ani_rid(A, v, a, b, c, d);
  if (ANI) return caltet_ani(a, b, c, d, smet(A, v[0]), smet(A, v[1]), smet(A, v[2]), smet(A, v[3]));
  return caltet_iso(a, b, c, d);
}

// log1p as glibc computes it (sysdeps/ieee754/dbl-64/s_log1p.c: Sun's fdlibm
// algorithm with its polynomial in the pairwise (Estrin) form glibc uses),
// restated so that the lengths are the reference's bit for bit on a glibc
// host -- ocml's log1p differs from it in the last ulp now and then.
// Checked against glibc 2.35's log1p on 5e7 inputs over (-0.49, 20) and
// tiny / huge ranges: no difference (tests/test_oracle.py pins the C twin of
// this code against the host's log1p).  Needs -ffp-contract=off (the
// library's flag): every product and sum rounded as in the C source.
static __device__ double pmx_log1p(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
               Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
               Lp7 = 1.479819860511658591e-01;
  double f = 0.0, c = 0.0, u;
  int hx = __double2hiint(x), hu = 0, k = 1;
  const int ax = hx & 0x7fffffff;
  if (hx < 0x3FDA827A) {                          // x < 0.41422
    if (ax >= 0x3ff00000) return x == -1.0 ? -__builtin_inf() : (x - x) / (x - x);   // x <= -1
    if (ax < 0x3e200000) return ax < 0x3c900000 ? x : x - x * x * 0.5;                // |x| < 2^-29
    if (hx > 0 || hx <= (int)0xbfd2bec3) { k = 0; f = x; hu = 1; }                     // -0.2929 < x < 0.41422
  } else if (hx >= 0x7ff00000) {
    return x + x;
  }
  if (k != 0) {
    if (hx < 0x43400000) {
      u = 1.0 + x;
      hu = __double2hiint(u);
      k = (hu >> 20) - 1023;
      c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);  // correction term
      c /= u;
    } else {
      u = x;
      hu = __double2hiint(u);
      k = (hu >> 20) - 1023;
      c = 0.0;
    }
    hu &= 0x000fffff;
    if (hu < 0x6a09e) {
      u = __hiloint2double(hu | 0x3ff00000, __double2loint(u));            // normalise u
    } else {
      k += 1;
      u = __hiloint2double(hu | 0x3fe00000, __double2loint(u));            // normalise u / 2
      hu = (0x00100000 - hu) >> 2;
    }
    f = u - 1.0;
  }
  const double hfsq = 0.5 * f * f;
  const double dk = (double)k;
  if (hu == 0) {                                   // |f| < 2^-20
    if (f == 0.0) {
      if (k == 0) return 0.0;
      c += dk * ln2_lo;
      return dk * ln2_hi + c;
    }
    const double R = hfsq * (1.0 - 0.66666666666666666 * f);
    if (k == 0) return f - R;
    return dk * ln2_hi - ((R - (dk * ln2_lo + c)) - f);
  }
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double R1 = z * Lp1, z2 = z * z, R2 = Lp2 + z * Lp3, z4 = z2 * z2, R3 = Lp4 + z * Lp5, z6 = z4 * z2,
               R4 = Lp6 + z * Lp7;
  const double R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
  if (k == 0) return f - (hfsq - s * (hfsq + R));
  return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + (dk * ln2_lo + c))) - f);
}

// MMG5_lenEdg_iso in two halves: the loads (the sizes issued with the
// coordinates -- the scheduler otherwise places them after the wait for the
// coordinates, a second round trip) and the arithmetic, so that a caller can
// put work between them
struct IsoEdge { D3 c1, c2; double h1, h2; };
__device__ __forceinline__ IsoEdge iso_edge_load(const StatArgs &A, int p1, int p2) {
  IsoEdge e;
  e.c1 = sld3(A, p1);
  e.c2 = sld3(A, p2);
  e.h1 = smet(A, p1)[0];
  e.h2 = smet(A, p2)[0];
  __builtin_amdgcn_sched_barrier(0);
  return e;
}
__device__ __forceinline__ double iso_edge_len(const IsoEdge &e) {
  double ux = e.c2.x - e.c1.x, uy = e.c2.y - e.c1.y, uz = e.c2.z - e.c1.z;
  double l = ux * ux + uy * uy + uz * uz;
  l = sqrt(l);
  double r = e.h2 / e.h1 - 1.0;
  // one division for both branches (l / h1 or l / (h2 - h1): the same
  // correctly rounded quotients as the two-branch form, one instead of two
  // in a wave whose lanes take both)
  const bool flat = fabs(r) < PMX_EPS;
  const double q = l / (flat ? e.h1 : (e.h2 - e.h1));
  return flat ? q : q * pmx_log1p(r);
}

// MMG5_lenEdg_iso / lenEdg33_ani (restated, unpinned; the surface lengths
// MMG5_lenSurfEdg_iso / lenSurfEdg33_ani of the parallel edges take the same
// formulas in classic metric storage)
template <bool ANI>
__device__ __forceinline__ double edge_len_t(const StatArgs &A, int p1, int p2) {
  if (ANI) {
    D3 c1 = sld3(A, p1), c2 = sld3(A, p2);
    double ux = c2.x - c1.x, uy = c2.y - c1.y, uz = c2.z - c1.z;
    const double *m1 = smet(A, p1), *m2 = smet(A, p2);
    double dd1 = mlen2(m1, ux, uy, uz);
    double dd2 = mlen2(m2, ux, uy, uz);
    if (dd1 <= 0.0) dd1 = 0.0;
    if (dd2 <= 0.0) dd2 = 0.0;
    return (sqrt(dd1) + sqrt(dd2) + 4.0 * sqrt(0.5 * (dd1 + dd2))) / 6.0;
  }
  const IsoEdge e = iso_edge_load(A, p1, p2);
  return iso_edge_len(e);
}
static __device__ double edge_len(const StatArgs &A, int p1, int p2) {
  return A.msize == 6 ? edge_len_t<true>(A, p1, p2) : edge_len_t<false>(A, p1, p2);
}

// MMG5_lenedg33_ani past its loads (edge_len_t<true>'s arithmetic)
__device__ __forceinline__ double ani_edge_len(D3 c1, D3 c2, const double *m1, const double *m2) {
  double ux = c2.x - c1.x, uy = c2.y - c1.y, uz = c2.z - c1.z;
  double dd1 = mlen2(m1, ux, uy, uz);
  double dd2 = mlen2(m2, ux, uy, uz);
  if (dd1 <= 0.0) dd1 = 0.0;
  if (dd2 <= 0.0) dd2 = 0.0;
  return (sqrt(dd1) + sqrt(dd2) + 4.0 * sqrt(0.5 * (dd1 + dd2))) / 6.0;
}

// ---- Mmg's surface-aware lengths in a tensor metric (restated from the public
// Mmg sources, unpinned; the oracle's orc_prilen_full, oracle/pmx_oracle_stats.c,
// is the same restatement in C).  The background's arrays: vbase 0, xstride 3.

// MG_SIN(tag) || (tag & MG_NOM): the stored metric is a plain tensor
__device__ __forceinline__ bool sin_or_nom(unsigned tg) { return (tg & (TAG_CRN | TAG_REQ | TAG_NOM)) != 0; }
__device__ __forceinline__ unsigned ptag_or0(const StatArgs &A, int ip) { return A.ptag ? A.ptag[ip] : 0u; }
// MMG5_Point.n (a ridge point's tangent, in mmg3d); zeros without surface data
__device__ __forceinline__ D3 pn_of(const StatArgs &A, int ip) {
  if (!A.pn) return D3{0.0, 0.0, 0.0};
  const double *r = A.pn + 3 * (int64_t)ip;
  return D3{r[0], r[1], r[2]};
}
// mesh->xpoint[p->xp].n1 / .n2 (entry 0: zeros)
__device__ __forceinline__ D3 xn_of(const StatArgs &A, int ip, int which) {
  if (!A.pxp) return D3{0.0, 0.0, 0.0};
  const double *r = A.xpn + 6 * (int64_t)A.pxp[ip] + 3 * which;
  return D3{r[0], r[1], r[2]};
}

// MMG5_buildridmet: ridge point np0's metric in the direction u, from its
// ridge storage m = (tangent size, in-surface sizes of sides 1 / 2, normal
// sizes of sides 1 / 2): the side whose normal is the more orthogonal to u,
// basis (t, n x t, n), mr = R diag(m0, dv, dn) R^T
static __device__ void buildridmet(const StatArgs &A, int np0, double ux, double uy, double uz, double mr[6]) {
  const double *m = smet(A, np0);
  const D3 t = pn_of(A, np0);
  D3 n1 = xn_of(A, np0, 0);
  const D3 n2 = xn_of(A, np0, 1);
  const double ps1 = ux * n1.x + uy * n1.y + uz * n1.z;
  const double ps2 = ux * n2.x + uy * n2.y + uz * n2.z;
  double dv, dn;
  if (fabs(ps2) < fabs(ps1)) {
    n1 = n2;
    dv = m[2];
    dn = m[4];
  } else {
    dv = m[1];
    dn = m[3];
  }
  double r[3][3];
  r[0][0] = t.x; r[1][0] = t.y; r[2][0] = t.z;
  r[0][1] = n1.y * t.z - n1.z * t.y;
  r[1][1] = n1.z * t.x - n1.x * t.z;
  r[2][1] = n1.x * t.y - n1.y * t.x;
  r[0][2] = n1.x; r[1][2] = n1.y; r[2][2] = n1.z;
  mr[0] = m[0] * r[0][0] * r[0][0] + dv * r[0][1] * r[0][1] + dn * r[0][2] * r[0][2];
  mr[1] = m[0] * r[0][0] * r[1][0] + dv * r[0][1] * r[1][1] + dn * r[0][2] * r[1][2];
  mr[2] = m[0] * r[0][0] * r[2][0] + dv * r[0][1] * r[2][1] + dn * r[0][2] * r[2][2];
  mr[3] = m[0] * r[1][0] * r[1][0] + dv * r[1][1] * r[1][1] + dn * r[1][2] * r[1][2];
  mr[4] = m[0] * r[1][0] * r[2][0] + dv * r[1][1] * r[2][1] + dn * r[1][2] * r[2][2];
  mr[5] = m[0] * r[2][0] * r[2][0] + dv * r[2][1] * r[2][1] + dn * r[2][2] * r[2][2];
}

// the tangent at ip of the curve under the edge [ip, ip + u] (MMG5_lenEdg's
// gammaprim): u at a singular / non-manifold point; along the point's tangent
// on a ridge edge (isedg); else u projected on the tangent plane of the side
// nearest to it (ridge point), of its xPoint normal (MG_REF), of its normal
static __device__ D3 gammaprim(const StatArgs &A, int ip, double ux, double uy, double uz, bool isedg) {
  const unsigned tg = ptag_or0(A, ip);
  if (sin_or_nom(tg)) return D3{ux, uy, uz};
  if (isedg) {
    const D3 t = pn_of(A, ip);
    const double ps1 = ux * t.x + uy * t.y + uz * t.z;
    return D3{ps1 * t.x, ps1 * t.y, ps1 * t.z};
  }
  D3 n1;
  double ps1;
  if (TAG_GEO & tg) {
    n1 = xn_of(A, ip, 0);
    const D3 n2 = xn_of(A, ip, 1);
    ps1 = ux * n1.x + uy * n1.y + uz * n1.z;
    const double ps2 = ux * n2.x + uy * n2.y + uz * n2.z;
    if (fabs(ps2) < fabs(ps1)) {
      n1 = n2;
      ps1 = ps2;
    }
  } else if (TAG_REF & tg) {
    n1 = xn_of(A, ip, 0);
    ps1 = ux * n1.x + uy * n1.y + uz * n1.z;
  } else {
    n1 = pn_of(A, ip);
    ps1 = ux * n1.x + uy * n1.y + uz * n1.z;
  }
  return D3{ux - ps1 * n1.x, uy - ps1 * n1.y, uz - ps1 * n1.z};
}

__device__ __forceinline__ double qform(const double *m, D3 g) {
  return m[0] * g.x * g.x + m[3] * g.y * g.y + m[5] * g.z * g.z + 2.0 * m[1] * g.x * g.y + 2.0 * m[2] * g.x * g.z +
         2.0 * m[4] * g.y * g.z;
}

// MMG5_lenSurfEdg33_ani (ridmet 0, classic storage) / MMG5_lenSurfEdg_ani
// (ridmet 1: a non-singular ridge endpoint's metric rebuilt per direction),
// both through MMG5_lenEdg: the mean of the end tangents' lengths, a negative
// quadratic form counting as 1
static __device__ double len_surf_ani(const StatArgs &A, int np0, int np1, bool isedg, bool ridmet) {
  const D3 c0 = sld3(A, np0), c1 = sld3(A, np1);
  const double ux = c1.x - c0.x, uy = c1.y - c0.y, uz = c1.z - c0.z;
  double m0[6], m1[6];
  const double *s0 = smet(A, np0), *s1 = smet(A, np1);
#pragma unroll
  for (int i = 0; i < 6; i++) { m0[i] = s0[i]; m1[i] = s1[i]; }
  if (ridmet) {
    const unsigned t0 = ptag_or0(A, np0), t1 = ptag_or0(A, np1);
    if (!sin_or_nom(t0) && (TAG_GEO & t0)) buildridmet(A, np0, ux, uy, uz, m0);
    if (!sin_or_nom(t1) && (TAG_GEO & t1)) buildridmet(A, np1, ux, uy, uz, m1);
  }
  const D3 g0 = gammaprim(A, np0, ux, uy, uz, isedg);
  const D3 g1 = gammaprim(A, np1, -ux, -uy, -uz, isedg);
  double l0 = qform(m0, g0), l1 = qform(m1, g1);
  if (l0 < 0.) l0 = 1.;
  if (l1 < 0.) l1 = 1.;
  return 0.5 * (sqrt(l0) + sqrt(l1));
}

// MMG5_moymet: the mean metric of tet v over its vertices that are not
// non-singular ridge points (false if none)
static __device__ bool moymet(const StatArgs &A, const int *v, double mm[6]) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) mm[i] = 0.0;
  for (int j = 0; j < 4; j++) {
    if (ridge_pt(ptag_or0(A, v[j]))) continue;
    n++;
    const double *m = smet(A, v[j]);
#pragma unroll
    for (int i = 0; i < 6; i++) mm[i] += m[i];
  }
  if (!n) return false;
  const double dd = 1. / n;
#pragma unroll
  for (int i = 0; i < 6; i++) mm[i] = mm[i] * dd;
  return true;
}

// MMG5_lenedg_ani (ridmet) / MMG5_lenedg33_ani of local edge ia = (ip1, ip2)
// of tet v (its packed xTetra edge tags et): a boundary edge of the xTetra along the
// surface, any other straight (MMG5_lenedgCoor_ani), a non-singular ridge
// endpoint then taking the tet's mean metric (MMG5_lenedgspl_ani)
static __device__ double len_tet_ani(const StatArgs &A, const int *v, int ia, int ip1, int ip2, unsigned et) {
  if ((et >> (2 * ia)) & 1u) return len_surf_ani(A, ip1, ip2, ((et >> (2 * ia + 1)) & 1u) != 0, A.ridmet != 0);
  double m1[6], m2[6];
  const double *s1 = smet(A, ip1), *s2 = smet(A, ip2);
#pragma unroll
  for (int i = 0; i < 6; i++) { m1[i] = s1[i]; m2[i] = s2[i]; }
  if (A.ridmet) {
    if (ridge_pt(ptag_or0(A, ip1)) && !moymet(A, v, m1)) return 0.0;
    if (ridge_pt(ptag_or0(A, ip2)) && !moymet(A, v, m2)) return 0.0;
  }
  const D3 c1 = sld3(A, ip1), c2 = sld3(A, ip2);
  const double ux = c2.x - c1.x, uy = c2.y - c1.y, uz = c2.z - c1.z;
  double dd1 = mlen2(m1, ux, uy, uz), dd2 = mlen2(m2, ux, uy, uz);
  if (dd1 <= 0.0) dd1 = 0.0;
  if (dd2 <= 0.0) dd2 = 0.0;
  return (sqrt(dd1) + sqrt(dd2) + 4.0 * sqrt(0.5 * (dd1 + dd2))) / 6.0;
}

// MMG5_lenSurfEdg_iso on a size-6 metric as the reference calls it for the
// parallel edges with metRidTyp = 1 (src/quality_pmmg.c:466): h = met->m[ip],
// the Mmg array (6 per point) read flat, i.e. component ip % 6 of point ip / 6
static __device__ double len_iso_flat(const StatArgs &A, int p1, int p2) {
  const D3 c1 = sld3(A, p1), c2 = sld3(A, p2);
  const double h1 = A.sol[(int64_t)(p1 / 6) * A.S + A.moff + p1 % 6];
  const double h2 = A.sol[(int64_t)(p2 / 6) * A.S + A.moff + p2 % 6];
  double l = (c2.x - c1.x) * (c2.x - c1.x) + (c2.y - c1.y) * (c2.y - c1.y) + (c2.z - c1.z) * (c2.z - c1.z);
  l = sqrt(l);
  const double r = h2 / h1 - 1.0;
  const bool flat = fabs(r) < PMX_EPS;
  const double q = l / (flat ? h1 : (h2 - h1));
  return flat ? q : q * pmx_log1p(r);
}
