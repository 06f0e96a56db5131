/*
 * metis_graph_demo.c -- PMMG_graph_meshElts2metis (reference
 * src/metis_pmmg.c:746-823) driven from plain C the way ParMmg's load
 * balancing would call it: upload the group, a count-only call for nadjncy,
 * allocate adjncy / adjwgt as the reference PMMG_CALLOCs them, the full call.
 *
 * Mesh: the jittered Kuhn cube n = 6 of the repository's generator
 * (parmmg_amd/csrc/meshgen.c, default seed), iso size h = (0.5 + 2 x) / n.
 * Prints "graph ne=.. nadjncy=.. adj=.. wgt=.." (FNV-1a sums of the arrays)
 * for tests/test_gpu_metis_graph.py to compare with Transfer.metis_graph, then
 * "graph ok".  Needs a GPU.
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

int main(void) {
  const int n = 6;
  int64_t np, ne, nt;
  pmg_kuhn_counts(n, &np, &ne, &nt);
  double *xyz = calloc((size_t)(np + 1) * 3, sizeof(double)), *h = calloc((size_t)np + 1, sizeof(double));
  int *tet = calloc((size_t)(ne + 1) * 4, sizeof(int)), *adja = calloc((size_t)(4 * ne + 5), sizeof(int));
  int *tria = calloc((size_t)(nt + 1) * 3, sizeof(int)), *adjt = calloc((size_t)(3 * nt + 4), sizeof(int));
  if (pmg_kuhn_cube(n, 20250117, 0.15, xyz, tet, adja, tria, adjt) != nt) return 1;
  h[0] = 1.0;
  for (int64_t i = 1; i <= np; i++) h[i] = (0.5 + 2.0 * xyz[3 * i]) / n;

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

  /* 1) count: xadj and nadjncy */
  int32_t *xadj = calloc((size_t)ne + 1, sizeof(int32_t));
  int64_t nadj = -1, nadj2 = -1;
  CK(pmx_metis_graph(ctx, 0, xadj, NULL, NULL, 0, &nadj));
  if (nadj != xadj[ne] || nadj <= 0 || nadj > 4 * ne) { fprintf(stderr, "count: %lld\n", (long long)nadj); return 1; }
  /* 2) allocate what the count asks for, fill */
  int32_t *adjncy = calloc((size_t)nadj, sizeof(int32_t)), *adjwgt = calloc((size_t)nadj, sizeof(int32_t));
  CK(pmx_metis_graph(ctx, 0, xadj, adjncy, adjwgt, nadj, &nadj2));
  if (nadj2 != nadj) { fprintf(stderr, "second count: %lld\n", (long long)nadj2); return 1; }
  for (int64_t c = 0; c < nadj; c++)
    if (adjncy[c] < 0 || adjncy[c] >= ne || adjwgt[c] < 1 || adjwgt[c] > 1000000) {
      fprintf(stderr, "entry %lld: %d %d\n", (long long)c, adjncy[c], adjwgt[c]);
      return 1;
    }
  /* one entry too few: refused, the count still reported */
  nadj2 = -1;
  if (pmx_metis_graph(ctx, 0, xadj, adjncy, adjwgt, nadj - 1, &nadj2) != 0 || nadj2 != nadj) {
    fprintf(stderr, "a short adjncy was not refused\n");
    return 1;
  }
  if (!(pmx_kernel_ms(ctx, 8) > 0.0)) { fprintf(stderr, "no kernel time\n"); return 1; }
  printf("graph ne=%lld nadjncy=%lld xadj=%016llx adj=%016llx wgt=%016llx\n", (long long)ne, (long long)nadj,
         (unsigned long long)fnv(xadj, ne + 1), (unsigned long long)fnv(adjncy, nadj),
         (unsigned long long)fnv(adjwgt, nadj));
  pmx_destroy(ctx);
  printf("graph ok\n");
  return 0;
}
