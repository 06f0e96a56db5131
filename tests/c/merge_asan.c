/* merge_asan.c -- the CPU twin of the group merge (merge_ref.c) driven end to end
 * on generated cubes, for an ASan/UBSan build (tests/test_merge_sanitizer.py):
 * the groups come from the split's twin (split_ref.c) -- z-slabs of the n = 3
 * cube in 2 and 3 parts, a pseudo-random five-part partition of the n = 6 cube
 * -- and are merged whole (no external communicator) and with the last group
 * left out as a remote rank (its positions the external communicators).  It
 * checks what can be checked without a second implementation: the sizes add
 * up, the maps and (group, old) are inverse to each other, and a refused call
 * writes nothing. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int64_t ne, np, nface, nnode; } spr_sizes;
int spr_split(int64_t ne, int64_t np, const int *tet, const int *adja, const int *part, int ngrp,
              int64_t nface_in, const int *face_in1, const int *face_in2,
              int64_t nnode_in, const int *node_in1, const int *node_in2,
              int64_t *int_face_nitem, int64_t *int_node_nitem,
              spr_sizes *sizes, int *tet_new, int *tet_old, int *tetra_v, int *adja_new, int *point_old,
              int *face1, int *face2, int *node1, int *node2);
typedef struct { int64_t np, ne, nnode, nface; } mgr_sizes;
int mgr_merge(int ngrp, const int64_t *poff, const int64_t *toff, const int64_t *noff, const int64_t *foff,
              const int *tet, const int *node1, const int *node2, const int *face1, const int *face2,
              int nsol, const int *sol_size, int64_t nitem_node, int64_t nitem_face,
              int next_node, const int64_t *node_off, const int *node_items,
              int next_face, const int64_t *face_off, const int *face_items,
              mgr_sizes *sizes, int *tetra_v, int *tet_group, int *tet_old, int *point_group, int *point_old,
              int *point_new, int *tet_new, int *out_node1, int *out_node2, int *out_face1, int *out_face2,
              int *ext_node_new, int *ext_face_new);
void pmg_kuhn_counts(int n, int64_t *np, int64_t *ne, int64_t *nt);
int64_t pmg_kuhn_cube(int n, uint64_t seed, double jitter, double *xyz, int *tet, int *adja, int *tria, int *adjt);

#define SENT (-77)

static int *ints(size_t n, int fill) {
  int *a = malloc(sizeof(int) * (n + 1));
  for (size_t i = 0; i <= n; i++) a[i] = fill;
  return a;
}

static int has(const int *a, int64_t lo, int64_t hi, int v) {
  for (int64_t i = lo; i < hi; i++)
    if (a[i] == v) return 1;
  return 0;
}

/* the cube of side n split by part into ngrp groups, its first `keep` groups merged */
static void run(int n, const int *part_of, int ngrp, int keep) {
  int64_t np, ne, nt;
  pmg_kuhn_counts(n, &np, &ne, &nt);
  double *xyz = malloc(sizeof(double) * 3 * (size_t)(np + 1));
  int *tet = ints(4 * (size_t)(ne + 1), 0), *adja = ints((size_t)(4 * ne + 5), 0);
  int *tria = ints(3 * (size_t)(nt + 1), 0), *adjt = ints((size_t)(3 * nt + 4), 0);
  if (pmg_kuhn_cube(n, 20250117u, 0.15, xyz, tet, adja, tria, adjt) != nt) exit(2);
  const size_t cap = (size_t)(4 * ne + 4);
  spr_sizes *ss = malloc(sizeof(spr_sizes) * (size_t)ngrp);
  int *s_tnew = ints((size_t)ne, 0), *s_told = ints((size_t)ne, 0), *s_tv = ints(4 * (size_t)ne, 0),
      *s_ad = ints(4 * (size_t)ne, 0), *s_pold = ints(cap, 0), *s_f1 = ints(cap, 0), *s_f2 = ints(cap, 0),
      *s_n1 = ints(cap, 0), *s_n2 = ints(cap, 0);
  int64_t fn = 0, nn = 0;
  if (!spr_split(ne, np, tet, adja, part_of, ngrp, 0, NULL, NULL, 0, NULL, NULL, &fn, &nn, ss, s_tnew, s_told, s_tv,
                 s_ad, s_pold, s_f1, s_f2, s_n1, s_n2))
    exit(3);
  /* the split's outputs are already concatenated in group order */
  int64_t *poff = calloc((size_t)ngrp + 1, sizeof(int64_t)), *toff = calloc((size_t)ngrp + 1, sizeof(int64_t)),
          *noff = calloc((size_t)ngrp + 1, sizeof(int64_t)), *foff = calloc((size_t)ngrp + 1, sizeof(int64_t));
  for (int g = 0; g < ngrp; g++) {
    poff[g + 1] = poff[g] + ss[g].np;
    toff[g + 1] = toff[g] + ss[g].ne;
    noff[g + 1] = noff[g] + ss[g].nnode;
    foff[g + 1] = foff[g] + ss[g].nface;
  }
  /* the positions the groups left out share with the ones kept */
  int *en = ints(cap, 0), *ef = ints(cap, 0);
  int64_t eoffn[2] = {0, 0}, eofff[2] = {0, 0};
  for (int64_t i = noff[keep]; i < noff[ngrp]; i++)
    if (has(s_n2, 0, noff[keep], s_n2[i]) && !has(en, 0, eoffn[1], s_n2[i])) en[eoffn[1]++] = s_n2[i];
  for (int64_t j = foff[keep]; j < foff[ngrp]; j++)
    if (has(s_f2, 0, foff[keep], s_f2[j])) ef[eofff[1]++] = s_f2[j];
  if (keep < ngrp && (eoffn[1] == 0 || eofff[1] == 0)) exit(4);
  const int64_t P = poff[keep], T = toff[keep];
  mgr_sizes ms = {SENT, SENT, SENT, SENT};
  int *tv = ints(4 * (size_t)T, SENT), *tg = ints((size_t)T, SENT), *to = ints((size_t)T, SENT),
      *pg = ints((size_t)P, SENT), *po = ints((size_t)P, SENT), *pn = ints((size_t)P, SENT), *tn = ints((size_t)T, SENT),
      *o_n1 = ints(cap, SENT), *o_n2 = ints(cap, SENT), *o_f1 = ints(cap, SENT), *o_f2 = ints(cap, SENT),
      *xn = ints(cap, SENT), *xf = ints(cap, SENT);
  const int next = keep < ngrp ? 1 : 0;
  /* a refused call first: an external node item out of range */
  if (next) {
    const int saved = en[0];
    en[0] = (int)nn;
    if (mgr_merge(keep, poff, toff, noff, foff, s_tv, s_n1, s_n2, s_f1, s_f2, 0, NULL, nn, fn, next, eoffn, en, next,
                  eofff, ef, &ms, tv, tg, to, pg, po, pn, tn, o_n1, o_n2, o_f1, o_f2, xn, xf))
      exit(5);
    if (ms.np != SENT || tv[0] != SENT || pn[0] != SENT || xn[0] != SENT) exit(6);
    en[0] = saved;
  }
  if (!mgr_merge(keep, poff, toff, noff, foff, s_tv, s_n1, s_n2, s_f1, s_f2, 0, NULL, nn, fn, next, eoffn, en, next,
                 eofff, ef, &ms, tv, tg, to, pg, po, pn, tn, o_n1, o_n2, o_f1, o_f2, xn, xf))
    exit(7);
  if (ms.ne != T || ms.np > P || ms.nface != eofff[1] || ms.nnode != eoffn[1]) exit(8);
  if (keep == ngrp && ms.np != np) exit(9);
  for (int64_t k = 0; k < ms.ne; k++)
    if (tn[toff[tg[k]] + to[k] - 1] != k + 1) exit(10);
  for (int64_t i = 0; i < ms.np; i++)
    if (pn[poff[pg[i]] + po[i] - 1] != i + 1) exit(11);
  for (int64_t i = 0; i < P; i++)
    if (pn[i] < 1 || pn[i] > ms.np) exit(12);
  free(xyz); free(tet); free(adja); free(tria); free(adjt); free(ss);
  free(s_tnew); free(s_told); free(s_tv); free(s_ad); free(s_pold); free(s_f1); free(s_f2); free(s_n1); free(s_n2);
  free(poff); free(toff); free(noff); free(foff); free(en); free(ef);
  free(tv); free(tg); free(to); free(pg); free(po); free(pn); free(tn);
  free(o_n1); free(o_n2); free(o_f1); free(o_f2); free(xn); free(xf);
}

int main(void) {
  int64_t np, ne, nt;
  pmg_kuhn_counts(3, &np, &ne, &nt);
  int *part = malloc(sizeof(int) * (size_t)ne);
  for (int ngrp = 2; ngrp <= 3; ngrp++) {
    /* contiguous runs of tet numbers: the generator numbers the cells layer by layer */
    for (int64_t k = 0; k < ne; k++) part[k] = (int)(k * ngrp / ne);
    run(3, part, ngrp, ngrp);
    run(3, part, ngrp, ngrp - 1);
  }
  run(3, part, 3, 1);
  free(part);
  pmg_kuhn_counts(6, &np, &ne, &nt);
  part = malloc(sizeof(int) * (size_t)ne);
  uint64_t s = 7;
  for (int64_t k = 0; k < ne; k++) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    part[k] = k < 5 ? (int)k : (int)((s >> 33) % 5);
  }
  run(6, part, 5, 5);
  run(6, part, 5, 4);
  free(part);
  printf("merge asan ok\n");
  return 0;
}
