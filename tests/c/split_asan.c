/* split_asan.c -- the CPU twin of the group split (split_ref.c) driven end to
 * end on generated cubes, for an ASan/UBSan build (tests/test_split_sanitizer.py):
 * z-slabs of the n = 3 cube (2 and 3 parts), a winding two-part partition and a
 * pseudo-random five-part one of the n = 6 cube, and a second split of a first
 * group fed with that group's communicators.  It checks what can be checked
 * without a second implementation: the sizes add up, every tet is placed once. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct { int64_t ne, np, nface, nnode; } spr_sizes;
int spr_split(int64_t ne, int64_t np, const int *tet, const int *adja, const int *part, int ngrp,
              int64_t nface_in, const int *face_in1, const int *face_in2,
              int64_t nnode_in, const int *node_in1, const int *node_in2,
              int64_t *int_face_nitem, int64_t *int_node_nitem,
              spr_sizes *sizes, int *tet_new, int *tet_old, int *tetra_v, int *adja_new, int *point_old,
              int *face1, int *face2, int *node1, int *node2);
void pmg_kuhn_counts(int n, int64_t *np, int64_t *ne, int64_t *nt);
int64_t pmg_kuhn_cube(int n, uint64_t seed, double jitter, double *xyz, int *tet, int *adja, int *tria, int *adjt);
int64_t pmg_build_adja(int64_t ne, const int *tet, int *adja);

typedef struct {
  int64_t np, ne;
  double *xyz;
  int *tet, *adja;
} Cube;

static Cube cube(int n) {
  Cube c;
  int64_t nt;
  pmg_kuhn_counts(n, &c.np, &c.ne, &nt);
  c.xyz = malloc(sizeof(double) * 3 * (size_t)(c.np + 1));
  c.tet = malloc(sizeof(int) * 4 * (size_t)(c.ne + 1));
  c.adja = malloc(sizeof(int) * (size_t)(4 * c.ne + 5));
  int *tria = malloc(sizeof(int) * 3 * (size_t)(nt + 1)), *adjt = malloc(sizeof(int) * (size_t)(3 * nt + 4));
  if (pmg_kuhn_cube(n, 20250117u, 0.15, c.xyz, c.tet, c.adja, tria, adjt) != nt) exit(2);
  free(tria);
  free(adjt);
  return c;
}

typedef struct {
  spr_sizes *sizes;
  int *tet_new, *tet_old, *tv, *ad, *pold, *f1, *f2, *n1, *n2;
  int64_t fn, nn;
} Out;

static Out run(int64_t ne, int64_t np, const int *tet, const int *adja, const int *part, int ngrp, int64_t nf,
               const int *if1, const int *if2, int64_t nnd, const int *in1, const int *in2, int64_t fn0, int64_t nn0) {
  Out o;
  const size_t cap = (size_t)(4 * ne + 4);
  o.sizes = malloc(sizeof(spr_sizes) * (size_t)ngrp);
  o.tet_new = malloc(sizeof(int) * (size_t)ne);
  o.tet_old = malloc(sizeof(int) * (size_t)ne);
  o.tv = malloc(sizeof(int) * 4 * (size_t)ne);
  o.ad = malloc(sizeof(int) * 4 * (size_t)ne);
  o.pold = malloc(sizeof(int) * cap);
  o.f1 = malloc(sizeof(int) * cap);
  o.f2 = malloc(sizeof(int) * cap);
  o.n1 = malloc(sizeof(int) * cap);
  o.n2 = malloc(sizeof(int) * cap);
  o.fn = fn0;
  o.nn = nn0;
  if (!spr_split(ne, np, tet, adja, part, ngrp, nf, if1, if2, nnd, in1, in2, &o.fn, &o.nn, o.sizes, o.tet_new,
                 o.tet_old, o.tv, o.ad, o.pold, o.f1, o.f2, o.n1, o.n2))
    exit(3);
  int64_t tets = 0, nodes = 0;
  for (int g = 0; g < ngrp; g++) {
    tets += o.sizes[g].ne;
    nodes += o.sizes[g].nnode;
    if (o.sizes[g].np < 4 || o.sizes[g].np > 4 * o.sizes[g].ne) exit(4);
  }
  if (tets != ne || o.nn != nn0 + nodes) exit(5);
  for (int64_t k = 1; k <= ne; k++) {
    int64_t off = 0;
    for (int g = 0; g < part[k - 1]; g++) off += o.sizes[g].ne;
    if (o.tet_old[off + o.tet_new[k - 1] - 1] != k) exit(6);
  }
  return o;
}

static void drop(Out *o) {
  free(o->sizes); free(o->tet_new); free(o->tet_old); free(o->tv); free(o->ad);
  free(o->pold); free(o->f1); free(o->f2); free(o->n1); free(o->n2);
}

static double zc(const Cube *c, int64_t k, int d) {
  double s = 0.0;
  for (int i = 0; i < 4; i++) s += c->xyz[3 * (int64_t)c->tet[4 * k + i] + d];
  return 0.25 * s;
}

int main(void) {
  /* case 1: z-slabs of the n = 3 cube, then group 0 split again with its communicators */
  Cube c = cube(3);
  int *part = malloc(sizeof(int) * (size_t)c.ne);
  for (int ngrp = 2; ngrp <= 3; ngrp++) {
    for (int64_t k = 1; k <= c.ne; k++) {
      int g = (int)(zc(&c, k, 2) * ngrp);
      part[k - 1] = g < ngrp ? g : ngrp - 1;
    }
    Out o = run(c.ne, c.np, c.tet, c.adja, part, ngrp, 0, NULL, NULL, 0, NULL, NULL, 0, 0);
    if (ngrp == 2) {
      const int64_t ne0 = o.sizes[0].ne, np0 = o.sizes[0].np;
      int *tet0 = calloc(4 * (size_t)(ne0 + 1), sizeof(int)), *adja0 = calloc((size_t)(4 * ne0 + 5), sizeof(int));
      int *part0 = malloc(sizeof(int) * (size_t)ne0);
      for (int64_t i = 0; i < 4 * ne0; i++) {
        tet0[4 + i] = o.tv[i];
        adja0[1 + i] = o.ad[i];
      }
      for (int64_t j = 1; j <= ne0; j++) part0[j - 1] = zc(&c, o.tet_old[j - 1], 0) < 0.5 ? 0 : 1;
      Out o2 = run(ne0, np0, tet0, adja0, part0, 2, o.sizes[0].nface, o.f1, o.f2, o.sizes[0].nnode, o.n1, o.n2,
                   o.fn, o.nn);
      if (o2.fn <= o.fn) exit(7);
      drop(&o2);
      free(tet0); free(adja0); free(part0);
    }
    drop(&o);
  }
  free(part);
  free(c.xyz); free(c.tet); free(c.adja);
  /* case 3: a winding interface and a pseudo-random assignment on the n = 6 cube */
  c = cube(6);
  part = malloc(sizeof(int) * (size_t)c.ne);
  for (int64_t k = 1; k <= c.ne; k++) {
    const int x = (int)(zc(&c, k, 0) * 6), y = (int)(zc(&c, k, 1) * 6), z = (int)(zc(&c, k, 2) * 6);
    part[k - 1] = (y % 2 == 0 && z % 2 == 0) || (y % 2 == 1 && z % 2 == 0 && x == ((y / 2) % 2 ? 0 : 5));
  }
  Out o = run(c.ne, c.np, c.tet, c.adja, part, 2, 0, NULL, NULL, 0, NULL, NULL, 0, 0);
  drop(&o);
  uint64_t s = 7;
  for (int64_t k = 1; k <= c.ne; k++) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    part[k - 1] = k <= 5 ? (int)(k - 1) : (int)((s >> 33) % 5);
  }
  o = run(c.ne, c.np, c.tet, c.adja, part, 5, 0, NULL, NULL, 0, NULL, NULL, 0, 0);
  drop(&o);
  free(part);
  free(c.xyz); free(c.tet); free(c.adja);
  printf("split asan ok\n");
  return 0;
}
