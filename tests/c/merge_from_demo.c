/*
 * merge_from_demo.c -- the second merge of PMMG_split_n2mGrps (reference
 * src/loadbalancing_pmmg.c:135) driven from plain C on one rank with its
 * groups on the device: a mesh is split in two (pmx_split_groups), each new
 * group becomes the background of a context of its own (pmx_split_adopt), and
 * pmx_merge_groups_from merges the two held groups -- only their communicator
 * index arrays come from the host.  The result is compared with
 * pmx_merge_groups of the same groups fetched to the host, then adopted.
 *
 * Mesh: the jittered Kuhn cube n = 6 of the repository's generator
 * (parmmg_amd/csrc/meshgen.c, default seed); part: tet i (0-based) in group
 * 2 i / ne.  Prints "merge_from np=.. ne=.. nnode=.. nface=.. tetra=..
 * tet_old=.. point_old=.." (FNV-1a sums of the arrays) for
 * tests/test_gpu_merge_from.py to recompute from the twin, then
 * "merge_from ok".  Needs a GPU.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pmx_transfer.h"

void pmg_kuhn_counts(int n, int64_t *np, int64_t *ne, int64_t *nt);
int64_t pmg_kuhn_cube(int n, uint64_t seed, double jitter, double *xyz, int *tet, int *adja, int *tria,
                      int *adjt);

static uint64_t fnv(const int32_t *a, int64_t n) {
  uint64_t h = 1469598103934665603ull;
  for (int64_t i = 0; i < n; i++) {
    h ^= (uint32_t)a[i];
    h *= 1099511628211ull;
  }
  return h;
}

#define CK(x) do { if (!(x)) { fprintf(stderr, "%s: %s\n", #x, pmx_last_error(ctx)); return 1; } } while (0)

typedef struct {
  int *tetra_v, *node1, *node2, *face1, *face2;
  double *xyz, *met;
} group_arrays;

int main(void) {
  const int n = 6;
  int64_t np, ne, nt;
  pmg_kuhn_counts(n, &np, &ne, &nt);
  double *xyz = calloc((size_t)(np + 1) * 3, sizeof(double)), *h = calloc((size_t)np + 1, sizeof(double));
  int *tet = calloc((size_t)(ne + 1) * 4, sizeof(int)), *adja = calloc((size_t)(4 * ne + 5), sizeof(int));
  int *tria = calloc((size_t)(nt + 1) * 3, sizeof(int)), *adjt = calloc((size_t)(3 * nt + 4), sizeof(int));
  if (pmg_kuhn_cube(n, 20250117, 0.15, xyz, tet, adja, tria, adjt) != nt) return 1;
  for (int64_t i = 0; i <= np; i++) h[i] = 1.0 + 0.001 * (double)i;

  pmx_ctx *ctx = pmx_create(0), *held[2] = {pmx_create(0), pmx_create(0)};
  if (!ctx || !held[0] || !held[1]) { fprintf(stderr, "no device\n"); return 1; }
  pmx_mesh_view v;
  memset(&v, 0, sizeof v);
  v.np = np; v.ne = ne; v.nt = nt;
  v.point_c = xyz; v.point_stride = 24;
  v.tetra_v = tet; v.tetra_stride = 16;
  v.adja = adja;
  v.tria_v = tria; v.tria_stride = 12;
  v.adjt = adjt;
  v.hausd = 0.01;
  pmx_sol_view met = {1, h};
  CK(pmx_upload_background(ctx, &v, 1, &met, 0));

  /* 1) the split, and each new group into a context of its own */
  int32_t *part = calloc((size_t)ne, sizeof(int32_t));
  int *tet_new = calloc((size_t)ne, sizeof(int));
  for (int64_t i = 0; i < ne; i++) part[i] = (int32_t)(2 * i / ne);
  pmx_split_sizes ss[2];
  int64_t nitem_face = -1, nitem_node = -1;
  CK(pmx_split_groups(ctx, part, 2, NULL, ss, tet_new, &nitem_face, &nitem_node));
  group_arrays ga[2];
  pmx_sol_view gmet[2];
  for (int g = 0; g < 2; g++) {
    ga[g].tetra_v = calloc((size_t)(ss[g].ne + 1) * 4, sizeof(int));
    ga[g].node1 = calloc((size_t)ss[g].nnode + 1, sizeof(int));
    ga[g].node2 = calloc((size_t)ss[g].nnode + 1, sizeof(int));
    ga[g].face1 = calloc((size_t)ss[g].nface + 1, sizeof(int));
    ga[g].face2 = calloc((size_t)ss[g].nface + 1, sizeof(int));
    ga[g].xyz = calloc((size_t)(ss[g].np + 1) * 3, sizeof(double));
    ga[g].met = calloc((size_t)ss[g].np + 1, sizeof(double));
    gmet[g].size = 1;
    gmet[g].m = ga[g].met;
    pmx_split_out o;
    memset(&o, 0, sizeof o);
    o.tetra_v = ga[g].tetra_v;
    o.node_index1 = ga[g].node1; o.node_index2 = ga[g].node2;
    o.face_index1 = ga[g].face1; o.face_index2 = ga[g].face2;
    o.xyz = ga[g].xyz;
    o.nsol = 1;
    o.sols = &gmet[g];
    CK(pmx_split_fetch(ctx, g, &o));
    if (!pmx_split_adopt(ctx, g, held[g], 0, 0, 0.01)) {
      fprintf(stderr, "pmx_split_adopt: %s\n", pmx_last_error(held[g]));
      return 1;
    }
  }

  /* 2) the merge of the two held groups: index arrays only */
  pmx_merge_source src[2];
  pmx_merge_group grp[2];
  memset(src, 0, sizeof src);
  memset(grp, 0, sizeof grp);
  for (int g = 0; g < 2; g++) {
    src[g].held = held[g];
    src[g].g.nnode = ss[g].nnode; src[g].g.nface = ss[g].nface;
    src[g].g.node_index1 = ga[g].node1; src[g].g.node_index2 = ga[g].node2;
    src[g].g.face_index1 = ga[g].face1; src[g].g.face_index2 = ga[g].face2;
    grp[g] = src[g].g;
    grp[g].np = ss[g].np; grp[g].ne = ss[g].ne;
    grp[g].point_c = ga[g].xyz; grp[g].point_stride = 24;
    grp[g].tetra_v = ga[g].tetra_v; grp[g].tetra_stride = 16;
    grp[g].sols = &gmet[g];
  }
  pmx_merge_comm comm;
  memset(&comm, 0, sizeof comm);
  comm.int_node_nitem = nitem_node;
  comm.int_face_nitem = nitem_face;
  pmx_merge_sizes ms, mh;
  CK(pmx_merge_groups_from(ctx, 2, src, 1, &comm, &ms));
  if (ms.np != np || ms.ne != ne) { fprintf(stderr, "merged %lld points, %lld tets\n", (long long)ms.np, (long long)ms.ne); return 1; }
  int *mt = calloc((size_t)(ne + 1) * 4, sizeof(int)), *told = calloc((size_t)ne, sizeof(int));
  int *pold = calloc((size_t)np, sizeof(int));
  int *mt2 = calloc((size_t)(ne + 1) * 4, sizeof(int)), *told2 = calloc((size_t)ne, sizeof(int));
  int *pold2 = calloc((size_t)np, sizeof(int));
  pmx_merge_out out;
  memset(&out, 0, sizeof out);
  out.tetra_v = mt; out.tet_old = told; out.point_old = pold;
  CK(pmx_merge_fetch(ctx, &out));
  /* the holders are not needed any more: the plan owns its copies */
  pmx_destroy(held[0]);
  pmx_destroy(held[1]);
  CK(pmx_merge_adopt(ctx, 0));
  if (!(pmx_kernel_ms(ctx, 16) > 0.0) || !(pmx_kernel_ms(ctx, 18) > 0.0)) { fprintf(stderr, "no kernel time\n"); return 1; }

  /* 3) the same groups from the host */
  CK(pmx_merge_groups(ctx, 2, grp, 1, &comm, &mh));
  out.tetra_v = mt2; out.tet_old = told2; out.point_old = pold2;
  CK(pmx_merge_fetch(ctx, &out));
  if (memcmp(&ms, &mh, sizeof ms) || memcmp(mt + 4, mt2 + 4, (size_t)ne * 16) || memcmp(told, told2, (size_t)ne * 4) ||
      memcmp(pold, pold2, (size_t)np * 4)) {
    fprintf(stderr, "held and host sources differ\n");
    return 1;
  }
  printf("merge_from np=%lld ne=%lld nnode=%lld nface=%lld tetra=%016llx tet_old=%016llx point_old=%016llx\n",
         (long long)ms.np, (long long)ms.ne, (long long)ms.nnode, (long long)ms.nface,
         (unsigned long long)fnv(mt + 4, 4 * ne), (unsigned long long)fnv(told, ne), (unsigned long long)fnv(pold, np));
  pmx_destroy(ctx);
  printf("merge_from ok\n");
  return 0;
}
