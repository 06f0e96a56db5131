/*
 * manyfields_demo.c -- ParMmg's two interpolation seams, as
 * integration/pmmg_pmx.c defines them (exact reference signatures), on one
 * group that carries more solution fields than the library's fused step
 * (mesh->nsols = 12 beside the metric; PMX_MAX_SOLS is 8):
 *
 *   src/libparmmg1.c:792  PMMG_copyMetricsAndFields_point
 *   src/libparmmg1.c:829  PMMG_interpMetricsAndFields
 *
 * The ParMmg structures come from the test-local tests/c/pmmg_stub/parmmg.h.
 * Inputs: raw arrays in <dir> written by tests/test_gpu_many_fields_binding.py
 * (sizes.txt: np ne np2 ne2 msize nfld, then the nfld field sizes;
 * old_{xyz,tet,tag,met}.bin, old_fld_<j>.bin, new_{xyz,tet,tag}.bin, all in
 * Mmg's 1-based layout); the background's boundary trias are built on the
 * device as adapter_demo.c does.  Outputs: <dir>/out_met.bin and
 * <dir>/out_fld_<j>.bin (every output array starts at -7), one JSON object
 * per call on stdout.
 *
 * usage: manyfields_demo <dir>
 */
#include "parmmg.h"
#include "pmx_transfer.h"

#define MAXF 64

static void *rd(const char *dir, const char *name, size_t bytes) {
  char path[1024];
  FILE *f;
  void *p = calloc(bytes ? bytes : 1, 1);
  snprintf(path, sizeof path, "%s/%s", dir, name);
  f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fclose(f);
  return p;
}
static void wr(const char *dir, const char *name, const void *p, size_t bytes) {
  char path[1024];
  FILE *f;
  snprintf(path, sizeof path, "%s/%s", dir, name);
  f = fopen(path, "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes || fclose(f) != 0) {
    fprintf(stderr, "cannot write %s\n", path);
    exit(2);
  }
}

/* the Mmg / ParMmg / MPI helpers the adapter's statistics seams link
 * against: never reached by the two interpolation seams */
static int unreachable(const char *who) {
  fprintf(stderr, "%s reached\n", who);
  exit(3);
}
int MMG3D_displayQualHisto_internal(int64_t ne, double max, double avg, double min, int iel, int good,
                                    int med, int his[PMMG_QUAL_HISSIZE], int nrid, int optimLES,
                                    int imprim) {
  (void)ne; (void)max; (void)avg; (void)min; (void)iel; (void)good; (void)med; (void)his; (void)nrid;
  (void)optimLES; (void)imprim;
  return unreachable(__func__);
}
int MMG5_displayLengthHisto_internal(int ned, int amin, int bmin, double lmin, int amax, int bmax,
                                     double lmax, int nullEdge, double *bd, int *hl, int8_t shift,
                                     int imprim) {
  (void)ned; (void)amin; (void)bmin; (void)lmin; (void)amax; (void)bmax; (void)lmax; (void)nullEdge;
  (void)bd; (void)hl; (void)shift; (void)imprim;
  return unreachable(__func__);
}
int PMMG_hashPar(MMG5_pMesh mesh, MMG5_HGeom *pHash) { (void)mesh; (void)pHash; return unreachable(__func__); }
int MMG5_hGet(MMG5_HGeom *hash, int a, int b, int *ref, int16_t *tag) {
  (void)hash; (void)a; (void)b; (void)ref; (void)tag;
  return unreachable(__func__);
}
int PMMG_build_edgeComm(PMMG_pParMesh parmesh, MMG5_pMesh mesh, MMG5_HGeom *hpar) {
  (void)parmesh; (void)mesh; (void)hpar;
  return unreachable(__func__);
}
void PMMG_edge_comm_free(PMMG_pParMesh parmesh) { (void)parmesh; unreachable(__func__); }
int MPI_Bcast(void *buf, int count, int type, int root, MPI_Comm comm) {
  (void)buf; (void)count; (void)type; (void)root; (void)comm;
  return unreachable(__func__);
}
int MPI_Allreduce(const void *sendbuf, void *recvbuf, int count, int type, int op, MPI_Comm comm) {
  (void)sendbuf; (void)recvbuf; (void)count; (void)type; (void)op; (void)comm;
  return unreachable(__func__);
}

static MMG5_pMesh make_mesh(int64_t np, int64_t ne, const double *xyz, const int *tet, const uint16_t *tag) {
  MMG5_pMesh m = calloc(1, sizeof *m);
  int64_t i;
  m->np = (int)np; m->ne = (int)ne;
  m->point = calloc((size_t)np + 1, sizeof(MMG5_Point));
  m->tetra = calloc((size_t)ne + 1, sizeof(MMG5_Tetra));
  for (i = 1; i <= np; i++) {
    memcpy(m->point[i].c, xyz + 3 * i, 3 * sizeof(double));
    m->point[i].tag = tag[i];
  }
  for (i = 1; i <= ne; i++) memcpy(m->tetra[i].v, tet + 4 * i, 4 * sizeof(int));
  m->info.hausd = 0.01;
  m->info.hsiz = 0.0;
  return m;
}

int main(int argc, char **argv) {
  const char *dir = argc > 1 ? argv[1] : ".";
  long long np, ne, np2, ne2;
  int msize, nfld, fsize[MAXF], ier, j;
  int64_t i, nt;
  char path[1024], name[64];
  FILE *f;
  MMG5_Sol oldfld[MAXF], fld[MAXF];
  snprintf(path, sizeof path, "%s/sizes.txt", dir);
  f = fopen(path, "r");
  if (!f || fscanf(f, "%lld %lld %lld %lld %d %d", &np, &ne, &np2, &ne2, &msize, &nfld) != 6) return 2;
  if (nfld < 1 || nfld > MAXF) return 2;
  for (j = 0; j < nfld; j++)
    if (fscanf(f, "%d", &fsize[j]) != 1) return 2;
  fclose(f);

  double *oxyz = rd(dir, "old_xyz.bin", (size_t)(np + 1) * 24);
  int *otet = rd(dir, "old_tet.bin", (size_t)(ne + 1) * 16);
  uint16_t *otag = rd(dir, "old_tag.bin", (size_t)(np + 1) * 2);
  double *omet = rd(dir, "old_met.bin", (size_t)(np + 1) * msize * 8);
  double *nxyz = rd(dir, "new_xyz.bin", (size_t)(np2 + 1) * 24);
  int *ntet = rd(dir, "new_tet.bin", (size_t)(ne2 + 1) * 16);
  uint16_t *ntag = rd(dir, "new_tag.bin", (size_t)(np2 + 1) * 2);

  /* the background group: its snapshot's boundary trias + adjacency, built
   * by the device builders (their own context) */
  MMG5_pMesh old = make_mesh(np, ne, oxyz, otet, otag);
  {
    pmx_ctx *topo = pmx_create(0);
    int *adja = calloc((size_t)(4 * ne + 5), sizeof(int));
    int *tria = calloc((size_t)(4 * ne + 1) * 3, sizeof(int));
    int *adjt = calloc((size_t)(12 * ne + 4), sizeof(int));
    if (!topo || !pmx_build_adja(topo, ne, np, otet, 16, adja)) return 4;
    nt = pmx_build_bdry(topo, ne, np, otet, 16, adja, tria, 4 * ne, adjt);
    if (nt < 0) return 4;
    old->nt = (int)nt;
    old->tria = calloc((size_t)nt + 1, sizeof(MMG5_Tria));
    for (i = 1; i <= nt; i++) memcpy(old->tria[i].v, tria + 3 * i, 3 * sizeof(int));
    old->adjt = adjt;
    old->adja = adja;
    free(tria);
    pmx_destroy(topo);
  }
  MMG5_pMesh mesh = make_mesh(np2, ne2, nxyz, ntet, ntag);
  mesh->nsols = nfld;
  old->nsols = nfld;
  MMG5_Sol oldmet = {(int)np, msize, omet};
  MMG5_Sol met = {(int)np2, msize, calloc((size_t)(np2 + 1) * msize, 8)};
  for (i = 0; i < (np2 + 1) * msize; i++) met.m[i] = -7.0;
  for (j = 0; j < nfld; j++) {
    snprintf(name, sizeof name, "old_fld_%d.bin", j);
    oldfld[j].np = (int)np; oldfld[j].size = fsize[j];
    oldfld[j].m = rd(dir, name, (size_t)(np + 1) * fsize[j] * 8);
    fld[j].np = (int)np2; fld[j].size = fsize[j];
    fld[j].m = calloc((size_t)(np2 + 1) * fsize[j], 8);
    for (i = 0; i < (np2 + 1) * fsize[j]; i++) fld[j].m[i] = -7.0;
  }

  PMMG_Grp grp, ogrp;
  memset(&grp, 0, sizeof grp);
  memset(&ogrp, 0, sizeof ogrp);
  grp.mesh = mesh; grp.met = &met; grp.field = fld;
  ogrp.mesh = old; ogrp.met = &oldmet; ogrp.field = oldfld;
  PMMG_ParMesh pm;
  memset(&pm, 0, sizeof pm);
  pm.myrank = 0; pm.nprocs = 1; pm.ngrp = 1;
  pm.listgrp = &grp; pm.old_listgrp = &ogrp;
  pm.info.imprim = 5; pm.info.imprim0 = 5; pm.info.root = 0; pm.info.inputMet = 1;

  /* src/libparmmg1.c:792 -- no device context exists yet */
  ier = PMMG_copyMetricsAndFields_point(mesh, old, &met, &oldmet, fld, oldfld, NULL, pm.info.inputMet);
  printf("{\"call\": \"copy\", \"ret\": %d}\n", ier);
  fflush(stdout);
  if (!ier) return 1;
  /* :829 */
  ier = PMMG_interpMetricsAndFields(&pm, NULL);
  printf("{\"call\": \"interp\", \"ret\": %d}\n", ier);
  fflush(stdout);
  if (!ier) return 1;
  wr(dir, "out_met.bin", met.m, (size_t)(np2 + 1) * msize * 8);
  for (j = 0; j < nfld; j++) {
    snprintf(name, sizeof name, "out_fld_%d.bin", j);
    wr(dir, name, fld[j].m, (size_t)(np2 + 1) * fsize[j] * 8);
  }
  return 0;
}
