/*
 * part_demo.c -- the partition stays on the device from the displacement's
 * marks to the split (PMMG_part_getInterfaces handed straight to
 * PMMG_split_grps, reference src/moveinterfaces_pmmg.c:1150-1212 and
 * src/grpsplit_pmmg.c:1680-1711), driven from plain C on one rank: upload the
 * group, begin, two layers, the fix and the reachability check on the device's
 * own marks, pmx_part_from_marks (DISTR target), release the displacement,
 * pmx_split_groups_part, fetch group 0.
 *
 * The same program runs the path this replaces -- pmx_moveifc_part into a host
 * array, pmx_split_groups of that array -- and compares: the group count, the
 * partition, every group's sizes, tet_new, both nitem and group 0's tet_old.
 * Any difference ends the program with a non-zero status.
 *
 * Mesh and old groups: those of moveifc_demo.c (the jittered Kuhn cube n = 6,
 * tet i in group 1 - 2 i / ne, weights 300 and 900).
 * Prints "part ok".  Needs a GPU.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pmx_transfer.h"

void pmg_kuhn_counts(int n, int64_t *np, int64_t *ne, int64_t *nt);
int64_t pmg_kuhn_cube(int n, uint64_t seed, double jitter, double *xyz, int *tet, int *adja, int *tria,
                      int *adjt);

#define CK(x) do { if (!(x)) { fprintf(stderr, "%s: %s\n", #x, pmx_last_error(ctx)); return 1; } } while (0)
#define SAME(x) do { if (!(x)) { fprintf(stderr, "the two paths differ: %s\n", #x); return 1; } } while (0)

int main(void) {
  const int n = 6, nold = 2;
  int64_t np, ne, nt;
  pmg_kuhn_counts(n, &np, &ne, &nt);
  double *xyz = calloc((size_t)(np + 1) * 3, sizeof(double)), *h = calloc((size_t)np + 1, sizeof(double));
  int *tet = calloc((size_t)(ne + 1) * 4, sizeof(int)), *adja = calloc((size_t)(4 * ne + 5), sizeof(int));
  int *tria = calloc((size_t)(nt + 1) * 3, sizeof(int)), *adjt = calloc((size_t)(3 * nt + 4), sizeof(int));
  if (pmg_kuhn_cube(n, 20250117, 0.15, xyz, tet, adja, tria, adjt) != nt) return 1;
  for (int64_t i = 0; i <= np; i++) h[i] = 1.0;

  pmx_ctx *ctx = pmx_create(0);
  if (!ctx) { fprintf(stderr, "no device\n"); return 1; }
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

  /* 1) the displacement: begin, two layers, the fix and the check in place */
  int32_t *tg = calloc((size_t)ne, sizeof(int32_t));
  for (int64_t i = 0; i < ne; i++) tg[i] = (int32_t)(1 - 2 * i / ne);
  const int displs[2] = {0, 2}, mapgrp[2] = {300, 900};
  const pmx_moveifc_map map = {1, 0, nold, displs, mapgrp};
  int64_t nfront = -1;
  CK(pmx_moveifc_begin(ctx, tg, &map, &nfront));
  for (int l = 0; l < 2; l++) CK(pmx_moveifc_layer(ctx, 0, NULL));
  pmx_contig_stats cs;
  pmx_reach_stats rs;
  CK(pmx_moveifc_fix(ctx, 0, &cs));
  CK(pmx_moveifc_reach(ctx, 0, NULL, NULL, 0, &rs));
  if (rs.counter != ne) { fprintf(stderr, "counter %lld\n", (long long)rs.counter); return 1; }

  /* 2) the path through the host's array, kept for the comparison */
  int32_t *part_h = calloc((size_t)ne, sizeof(int32_t)), *part_d = calloc((size_t)ne, sizeof(int32_t));
  int *tet_new_h = calloc((size_t)ne, sizeof(int)), *tet_new_d = calloc((size_t)ne, sizeof(int));
  int *old_h = calloc((size_t)ne, sizeof(int)), *old_d = calloc((size_t)ne, sizeof(int));
  int32_t ngrp_h = -1, ngrp_d = -1, ngrp_dl = -1, gmark[2] = {-1, -1};
  CK(pmx_moveifc_part(ctx, NULL, PMX_GRPSPL_DISTR_TARGET, NULL, part_h, &ngrp_h));

  /* 3) the partition on the device; the marks may go once it is read off them */
  if (pmx_kernel_ms(ctx, 24) != -1.0) { fprintf(stderr, "a kernel time before the call\n"); return 1; }
  CK(pmx_part_from_marks(ctx, PMX_GRPSPL_DISTR_TARGET, NULL, &ngrp_d, gmark));
  if (!(pmx_kernel_ms(ctx, 24) > 0.0)) { fprintf(stderr, "no kernel time\n"); return 1; }
  CK(pmx_moveifc_release(ctx));
  SAME(ngrp_d == ngrp_h && ngrp_d >= 1 && ngrp_d <= nold);
  /* one rank: the owner of every new group is rank 0, its mark the old group */
  for (int g = 0; g < ngrp_d; g++) SAME(gmark[g] >= 0 && gmark[g] < nold);
  CK(pmx_part_download(ctx, part_d, &ngrp_dl));
  SAME(ngrp_dl == ngrp_d && memcmp(part_d, part_h, sizeof(int32_t) * (size_t)ne) == 0);

  /* 4) the split by it, and group 0 */
  pmx_split_sizes sizes_d[2], sizes_h[2];
  int64_t nface_d = -1, nnode_d = -1, nface_h = -2, nnode_h = -2, sum = 0;
  CK(pmx_split_groups_part(ctx, NULL, sizes_d, tet_new_d, &nface_d, &nnode_d));
  pmx_split_out out;
  memset(&out, 0, sizeof out);
  out.tet_old = old_d;
  CK(pmx_split_fetch(ctx, 0, &out));

  /* 5) the same through the host's array */
  CK(pmx_split_groups(ctx, part_h, ngrp_h, NULL, sizes_h, tet_new_h, &nface_h, &nnode_h));
  out.tet_old = old_h;
  CK(pmx_split_fetch(ctx, 0, &out));
  for (int g = 0; g < ngrp_d; g++) {
    SAME(sizes_d[g].ne == sizes_h[g].ne && sizes_d[g].np == sizes_h[g].np);
    SAME(sizes_d[g].nface == sizes_h[g].nface && sizes_d[g].nnode == sizes_h[g].nnode);
    sum += sizes_d[g].ne;
  }
  SAME(sum == ne && nface_d == nface_h && nnode_d == nnode_h);
  SAME(memcmp(tet_new_d, tet_new_h, sizeof(int) * (size_t)ne) == 0);
  SAME(memcmp(old_d, old_h, sizeof(int) * (size_t)sizes_d[0].ne) == 0);
  printf("part ne=%lld ngrp=%d ne0=%lld\n", (long long)ne, ngrp_d, (long long)sizes_d[0].ne);

  /* the partition outlives the displacement and the split; an upload drops it */
  CK(pmx_part_download(ctx, part_d, NULL));
  CK(pmx_upload_background(ctx, &v, 1, &met, 0));
  if (pmx_part_download(ctx, part_d, NULL) != 0) { fprintf(stderr, "the upload kept the partition\n"); return 1; }
  pmx_destroy(ctx);
  printf("part ok\n");
  return 0;
}
