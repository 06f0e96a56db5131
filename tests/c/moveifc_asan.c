/* moveifc_asan.c -- the CPU twin of the interface displacement (moveifc_ref.c)
 * driven end to end on generated cubes, for an ASan/UBSan build
 * (tests/test_moveifc_sanitizer.py): a quadrant partition with the lighter
 * groups later (the front moves), a pseudo-random five-colour partition with
 * the tet counts as weights (balls abandoned at nemin), and three emulated
 * ranks whose node points are fed foreign colours before every layer.  It
 * checks what can be checked without a second implementation: no tet's weight
 * increases, negrp stays at or above nemin, the next front is what the layer
 * reports, and both targets of the partition read-out cover every tet. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  int nprocs, myrank, nold_grp;
  const int *displsgrp, *mapgrp;
} mir_map;
typedef struct {
  int64_t front, touched, recolor, next, blocks, maxball, overflow_ip;
} mir_stats;
int64_t mir_begin(int64_t ne, int64_t np, const int *tet, const mir_map *m, const int *tet_group, int *mark, int *tmp,
                  int *s, int *flag, int *negrp, int *nemin);
void mir_set_colors(int64_t n, const int *ip, const int *color, int *tmp, int *flag);
int mir_layer(int64_t ne, int64_t np, const int *tet, const int *adja, const mir_map *m, int *mark, int *tmp, int *s,
              int *flag, int *negrp, int *nemin, mir_stats *st);
int mir_part(int64_t ne, const int *mark, int nprocs, int myrank, int nold_grp, int target, const int *ngrps, int *part,
             int *ngrp);
void pmg_kuhn_counts(int n, int64_t *np, int64_t *ne, int64_t *nt);
int64_t pmg_kuhn_cube(int n, uint64_t seed, double jitter, double *xyz, int *tet, int *adja, int *tria, int *adjt);

static int *ints(size_t n) { return calloc(n + 1, sizeof(int)); }

static void fail(const char *what) {
  fprintf(stderr, "moveifc asan: %s\n", what);
  exit(1);
}

static int weight(const mir_map *m, int c) { return m->mapgrp[c / m->nprocs + m->displsgrp[c % m->nprocs]]; }

/* kind 0: quadrants, 1: pseudo-random five colours with counts as weights,
 * 2: z-slabs on rank 1 of 3 with foreign colours offered on the face x = 0 */
static void run(int n, int kind, int nlayers) {
  int64_t np, ne, nt;
  pmg_kuhn_counts(n, &np, &ne, &nt);
  double *xyz = malloc(sizeof(double) * 3 * (size_t)(np + 1));
  int *tet = ints(4 * (size_t)(ne + 1)), *adja = ints((size_t)(4 * ne + 5));
  int *tria = ints(3 * (size_t)(nt + 1)), *adjt = ints((size_t)(3 * nt + 4));
  if (pmg_kuhn_cube(n, 20250117u, 0.15, xyz, tet, adja, tria, adjt) != nt) exit(2);
  int *tg = ints((size_t)ne), *mark = ints((size_t)ne + 1), *before = ints((size_t)ne + 1);
  int *tmp = ints((size_t)np + 1), *s = ints((size_t)np + 1), *flag = ints((size_t)np + 1);
  int *part = ints((size_t)ne), *pts = ints((size_t)np), *col = ints((size_t)np);
  int displs[4] = {0, 0, 0, 0}, mapgrp[8] = {0}, negrp[8], nemin[8], ngrps[3];
  mir_map m = {1, 0, 0, displs, mapgrp};
  uint64_t rng = 88172645463325252ull;
  for (int64_t k = 1; k <= ne; k++) {
    double c[3] = {0, 0, 0};
    for (int j = 0; j < 4; j++)
      for (int a = 0; a < 3; a++) c[a] += xyz[3 * (size_t)tet[4 * k + j] + a] / 4;
    const int x = (int)(c[0] * n), y = (int)(c[1] * n), z = (int)(c[2] * n);
    rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
    tg[k - 1] = kind == 0 ? (x >= n / 2) + 2 * (y >= n / 2) : kind == 1 ? (int)(rng % 5) : (3 * z) / n;
  }
  if (kind == 2) {
    const int d[4] = {0, 1, 4, 6}, w[6] = {300, 0, 0, 0, 10, 600};
    m.nprocs = 3, m.myrank = 1, m.nold_grp = 3;
    memcpy(displs, d, sizeof d);
    memcpy(mapgrp, w, sizeof w);
    for (int64_t k = 0; k < ne; k++) mapgrp[1 + tg[k]]++;
  } else {
    m.nold_grp = kind == 0 ? 4 : 5;
    displs[1] = m.nold_grp;
    if (kind == 0) {
      const int w[4] = {900, 500, 500, 200};
      memcpy(mapgrp, w, sizeof w);
    } else
      for (int64_t k = 0; k < ne; k++) mapgrp[tg[k]]++;
  }
  int64_t npts = 0;
  for (int64_t p = 1; p <= np; p++)
    if (kind == 2 && xyz[3 * p] == 0.0) pts[npts++] = (int)p;
  int64_t nfront = mir_begin(ne, np, tet, &m, tg, mark, tmp, s, flag, negrp, nemin);
  int64_t blocks = 0, recolor = 0;
  for (int l = 0; l < nlayers; l++) {
    const int foreign[3] = {0, 2, 5};
    for (int64_t i = 0; i < npts; i++) {
      const int c = foreign[(i / 3 + l) % 3];
      col[i] = ((i + l) % 3 == 0 && weight(&m, c) < weight(&m, tmp[pts[i]])) ? c : tmp[pts[i]];
    }
    mir_set_colors(npts, pts, col, tmp, flag);
    memcpy(before, mark, sizeof(int) * (size_t)(ne + 1));
    mir_stats st;
    if (!mir_layer(ne, np, tet, adja, &m, mark, tmp, s, flag, negrp, nemin, &st)) fail("overflow on a cube");
    int64_t next = 0;
    for (int64_t k = 1; k <= ne; k++)
      if (weight(&m, mark[k]) > weight(&m, before[k])) fail("a tet's weight increased");
    for (int64_t p = 1; p <= np; p++) {
      if (flag[p] != 0 && flag[p] != 1) fail("a flag other than 0 / 1 between layers");
      if (s[p] < 4 || s[p] > 4 * ne + 3 || tet[s[p]] != p) fail("s is not a slot of its point");
      next += flag[p];
    }
    if (next != st.next) fail("next front");
    for (int g = 0; g < m.nold_grp; g++)
      if (negrp[g] < nemin[g]) fail("negrp below nemin");
    blocks += st.blocks;
    recolor += st.recolor;
  }
  if (kind == 1 && !blocks) fail("the counts-as-weights case did not block");
  if (kind != 1 && !recolor) fail("nothing moved");
  int ngrp = -1;
  for (int i = 0; i < m.nprocs; i++) ngrps[i] = displs[i + 1] - displs[i];
  if (!mir_part(ne, mark, m.nprocs, m.myrank, m.nold_grp, 1, ngrps, part, &ngrp) || ngrp < 1) fail("DISTR target");
  for (int64_t k = 0; k < ne; k++)
    if (part[k] < 0 || part[k] >= ngrp) fail("part out of range");
  const int ok = mir_part(ne, mark, m.nprocs, m.myrank, m.nold_grp, 2, ngrps, part, &ngrp);
  if (kind == 2 ? ok : !ok || ngrp != m.nold_grp) fail("MMG target");
  printf("n %d kind %d: front %lld, %lld recolourings, %lld blocks\n", n, kind, (long long)nfront, (long long)recolor,
         (long long)blocks);
  free(xyz), free(tet), free(adja), free(tria), free(adjt), free(tg), free(mark), free(before), free(tmp), free(s);
  free(flag), free(part), free(pts), free(col);
}

int main(void) {
  run(6, 0, 4);
  run(4, 1, 3);
  run(6, 1, 3);
  run(6, 2, 3);
  printf("moveifc asan ok\n");
  return 0;
}
