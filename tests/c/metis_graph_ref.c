/* CPU twin of pmx_metis_graph / pmx_face_weights (test infrastructure): the
 * semantics of PMMG_graph_meshElts2metis and PMMG_computeWgt (reference
 * src/metis_pmmg.c:746-823, :280-301) in plain C with glibc's log1p / exp,
 * for meshes without surface data:
 *   msize 1: MMG5_lenedg_iso (either metRidTyp);
 *   msize 6, ridmet 0: MMG5_lenedg33_ani;
 *   msize 6, ridmet 1: MMG5_lenedg_ani -- a non-singular ridge endpoint takes
 *     the mean metric of the tet's vertices that are not such points
 *     (MMG5_moymet; none: length 0);
 *   msize 0: no metric, every weight 1000000.
 * Arrays are Mmg's: 1-based, xyz (np+1) x 3, tet (ne+1) x 4, adja 4 ne + 5,
 * met (np+1) x msize, tag np+1 (or NULL).
 * Build: gcc -O3 -ffp-contract=off -shared -fPIC. */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

#define EPS 1.e-6
#define HUGEINT 1000000.0
#define TAG_GEO 2
#define TAG_REQ 4
#define TAG_NOM 8
#define TAG_CRN 32

static const int IARE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
static const int IARF[4][3] = {{5, 4, 3}, {5, 1, 2}, {4, 2, 0}, {3, 0, 1}};

typedef struct {
  const double *xyz, *met;
  const int *tet;
  const uint16_t *tag;
  int msize, ridmet;
} gctx;

static int ridge_pt(const gctx *g, int ip) {
  const unsigned tg = g->tag ? g->tag[ip] : 0u;
  const int sin = (tg & TAG_CRN) || (tg & TAG_REQ);
  return !(sin || (tg & TAG_NOM)) && (tg & TAG_GEO);
}

static double mlen2(const double *m, double x, double y, double z) {
  return m[0] * x * x + m[3] * y * y + m[5] * z * z + 2.0 * (m[1] * x * y + m[2] * x * z + m[4] * y * z);
}

static int moymet(const gctx *g, const int *v, double mm[6]) {
  int i, j, n = 0;
  double dd;
  for (i = 0; i < 6; i++) mm[i] = 0.0;
  for (j = 0; j < 4; j++) {
    if (ridge_pt(g, v[j])) continue;
    n++;
    for (i = 0; i < 6; i++) mm[i] += g->met[6 * (int64_t)v[j] + i];
  }
  if (!n) return 0;
  dd = 1. / n;
  for (i = 0; i < 6; i++) mm[i] = mm[i] * dd;
  return 1;
}

/* MMG5_lenedg(mesh, met, ia, pt) of tet k */
static double lenedg(const gctx *g, int64_t k, int ia) {
  const int *v = g->tet + 4 * k;
  const int p1 = v[IARE[ia][0]], p2 = v[IARE[ia][1]];
  const double *c1 = g->xyz + 3 * (int64_t)p1, *c2 = g->xyz + 3 * (int64_t)p2;
  const double ux = c2[0] - c1[0], uy = c2[1] - c1[1], uz = c2[2] - c1[2];
  if (g->msize == 1) {
    const double h1 = g->met[p1], h2 = g->met[p2];
    double l = ux * ux + uy * uy + uz * uz, r;
    l = sqrt(l);
    r = h2 / h1 - 1.0;
    return (fabs(r) < EPS) ? (l / h1) : (l / (h2 - h1) * log1p(r));
  } else {
    double m1[6], m2[6], dd1, dd2;
    int i;
    for (i = 0; i < 6; i++) {
      m1[i] = g->met[6 * (int64_t)p1 + i];
      m2[i] = g->met[6 * (int64_t)p2 + i];
    }
    if (g->ridmet) {
      if (ridge_pt(g, p1) && !moymet(g, v, m1)) return 0.0;
      if (ridge_pt(g, p2) && !moymet(g, v, m2)) return 0.0;
    }
    dd1 = mlen2(m1, ux, uy, uz);
    dd2 = mlen2(m2, ux, uy, uz);
    if (dd1 <= 0.0) dd1 = 0.0;
    if (dd2 <= 0.0) dd2 = 0.0;
    return (sqrt(dd1) + sqrt(dd2) + 4.0 * sqrt(0.5 * (dd1 + dd2))) / 6.0;
  }
}

/* PMMG_computeWgt; len4 (or NULL) receives the face's three lengths and the
 * weight before MG_MIN clamps it */
static double compute_wgt(const gctx *g, int64_t k, int ifac, double *len4) {
  const double alpha = 28.0;
  double res, len;
  int i;
  if (g->msize == 0) {
    if (len4) len4[0] = len4[1] = len4[2] = len4[3] = HUGEINT;
    return HUGEINT;
  }
  res = 0.0;
  for (i = 0; i < 3; i++) {
    len = lenedg(g, k, IARF[ifac][i]);
    if (len4) len4[i] = len;
    if (len <= 1.0) res += len - 1.0;
    else res += 1.0 / len - 1.0;
  }
  res = 1.0 / exp(alpha * res / 3.0);
  if (len4) len4[3] = res;
  return res < HUGEINT ? res : HUGEINT;
}

/* The graph: xadj ne+1; adjncy / wgt / iwgt / len (4 per entry) 4 ne entries
 * each, any of the last three may be NULL.  Returns nadjncy. */
int64_t mgr_graph(int64_t ne, const double *xyz, const int *tet, const int *adja, const double *met, int msize,
                  int ridmet, const uint16_t *tag, int32_t *xadj, int32_t *adjncy, double *wgt, int32_t *iwgt,
                  double *len) {
  gctx g = {xyz, met, tet, tag, met ? msize : 0, ridmet && msize == 6};
  int64_t k, count = 0;
  int j;
  xadj[0] = 0;
  for (k = 1; k <= ne; k++) {
    const int *a = adja + 4 * (k - 1) + 1;
    for (j = 0; j < 4; j++) {
      const int jel = a[j] / 4;
      double w;
      if (!jel) continue;
      if (wgt || iwgt || len) {
        w = compute_wgt(&g, k, j, len ? len + 4 * count : NULL);
        if (wgt) wgt[count] = w;
        if (iwgt) iwgt[count] = (int)w > 1 ? (int)w : 1;
      }
      adjncy[count++] = jel - 1;
    }
    xadj[k] = (int32_t)count;
  }
  return count;
}

/* PMMG_computeWgt of n listed faces, face[i] = 12 ie + 3 ifac (+ iloc) */
void mgr_face_weights(const double *xyz, const int *tet, const double *met, int msize, int ridmet,
                      const uint16_t *tag, int64_t n, const int *face, double *wgt) {
  gctx g = {xyz, met, tet, tag, met ? msize : 0, ridmet && msize == 6};
  int64_t i;
  for (i = 0; i < n; i++) wgt[i] = compute_wgt(&g, face[i] / 12, (face[i] % 12) / 3, NULL);
}
