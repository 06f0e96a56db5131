/* merge_ref.c -- CPU twin of pmx_merge_groups / pmx_merge_fetch / pmx_merge_maps
 * (test infrastructure, tests/merge_ref.py).
 *
 * The passes of PMMG_merge_grps (reference src/mergemesh_pmmg.c:967-1073) on
 * packed groups, restated on flat arrays with the reference's own bookkeeping:
 * the two intvalues arrays, the tmp of every point, flag and base of every
 * tet, and counters that run in the reference's order -- group 0's face and
 * node entries stored, the interface points of the groups 1.. (:303-403), then
 * per group its internal points (:480-571), its interface tets (:584-682) and
 * its internal tets (:695-751), then the node and the face communicators
 * walked over the external ones (:763-935).  Nothing here ranks, sorts or
 * scans: it is written independently of the device derivation (DESIGN.md
 * section 4, "Group merge") so that the two can be compared.
 *
 * UNPINNED: Mmg is absent here, so the reference cannot be built.  Assumption:
 * on a packed mesh MMG3D_newPt and MMG3D_newElt hand out np + 1 and ne + 1.
 * Not restated: xPoint / xTetra copies, ref, tag, qual, n (they follow the
 * maps), PMMG_updateTag, the reallocation of the communicator arrays.  tet_new
 * holds the merged tet of every input tet; the reference keeps it in
 * tetra[k].flag for the interface tets only.  The reference returns early
 * when ngrp == 1; here one group goes through the same passes as several.
 *
 * The groups come concatenated: points, tets (4 ints each, group-local vertex
 * ids), node entries and face entries of group g at poff / toff / noff /
 * foff [g] .. [g + 1].  Every refusal returns 0 before an output is written. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int64_t np, ne, nnode, nface; } mgr_sizes;

static const char *mgr_err = "";
const char *mgr_last_error(void) { return mgr_err; }

static int refuse(const char *why) {
  mgr_err = why;
  return 0;
}

int mgr_merge(int ngrp, const int64_t *poff, const int64_t *toff, const int64_t *noff, const int64_t *foff,
              const int *tet, const int *node1, const int *node2, const int *face1, const int *face2,
              int nsol, const int *sol_size, int64_t nitem_node, int64_t nitem_face,
              int next_node, const int64_t *node_off, const int *node_items,
              int next_face, const int64_t *face_off, const int *face_items,
              mgr_sizes *sizes, int *tetra_v, int *tet_group, int *tet_old, int *point_group, int *point_old,
              int *point_new, int *tet_new, int *out_node1, int *out_node2, int *out_face1, int *out_face2,
              int *ext_node_new, int *ext_face_new) {
  /* ---- what the reference asserts or presupposes ---- */
  if (ngrp < 1) return refuse("ngrp < 1");
  if (!poff || !toff || !noff || !foff || !tet) return refuse("a NULL view");
  if (nsol < 0 || nsol > 8) return refuse("nsol outside 0..PMX_MAX_SOLS");
  if (nsol > 0 && !sol_size) return refuse("a NULL view");
  for (int g = 1; g < ngrp; g++)
    for (int i = 0; i < nsol; i++)
      if (sol_size[g * nsol + i] != sol_size[i]) return refuse("solution sizes differ between groups");
  const int64_t P = poff[ngrp], T = toff[ngrp], NN = noff[ngrp], NF = foff[ngrp];
  if ((NN > 0 && (!node1 || !node2)) || (NF > 0 && (!face1 || !face2))) return refuse("a NULL view");
  if (P >= 2147483647LL) return refuse("the groups' points together >= 2^31 - 1");
  if (12 * T + 11 >= 2147483648LL) return refuse("12 ne + 11 >= 2^31");
  for (int g = 0; g < ngrp; g++) {
    const int64_t npg = poff[g + 1] - poff[g], neg = toff[g + 1] - toff[g];
    if (npg < 1 || neg < 1) return refuse("a NULL view");
    for (int64_t k = toff[g]; k < toff[g + 1]; k++) {
      if (tet[4 * k] <= 0) return refuse("a deleted tet");
      for (int l = 0; l < 4; l++)
        if (tet[4 * k + l] < 1 || tet[4 * k + l] > npg) return refuse("a vertex outside 1..np");
    }
    for (int64_t i = noff[g]; i < noff[g + 1]; i++) {
      if (node1[i] < 1 || node1[i] > npg) return refuse("a node entry's point outside 1..np");
      if (node2[i] < 0 || node2[i] >= nitem_node) return refuse("a node entry's position out of range");
    }
    for (int64_t j = foff[g]; j < foff[g + 1]; j++) {
      if (face1[j] < 12 || face1[j] > 12 * neg + 11) return refuse("a face entry outside 12..12*ne+11");
      if (face2[j] < 0 || face2[j] >= nitem_face) return refuse("a face entry's position out of range");
    }
  }
  const int64_t NEN = next_node > 0 ? node_off[next_node] : 0, NEF = next_face > 0 ? face_off[next_face] : 0;
  if ((NEN > 0 && !node_items) || (NEF > 0 && !face_items)) return refuse("a NULL view");
  for (int64_t e = 0; e < NEN; e++)
    if (node_items[e] < 0 || node_items[e] >= nitem_node) return refuse("an external node item out of range");
  for (int64_t e = 0; e < NEF; e++)
    if (face_items[e] < 0 || face_items[e] >= nitem_face) return refuse("an external face item out of range");

  /* ---- the working state: nothing of the caller's is written before the end ---- */
  int *ivn = calloc((size_t)nitem_node + 1, sizeof(int)), *ivf = calloc((size_t)nitem_face + 1, sizeof(int));
  int *tmp = calloc((size_t)P + 1, sizeof(int));          /* point[k].tmp, group g's point k at poff[g] + k - 1 */
  int *flag = calloc((size_t)T + 1, sizeof(int));         /* tetra[k].flag */
  char *base = calloc((size_t)T + 1, 1);                  /* tetra[k].base == mesh->base */
  int *mv = malloc(sizeof(int) * 4 * (size_t)T), *mg = malloc(sizeof(int) * (size_t)T),
      *mo = malloc(sizeof(int) * (size_t)T);              /* merged tets: vertices, source group, local id */
  int *pg = malloc(sizeof(int) * (size_t)P), *po = malloc(sizeof(int) * (size_t)P);   /* merged points' sources */
  int *n1 = malloc(sizeof(int) * ((size_t)NEN + 1)), *n2 = malloc(sizeof(int) * ((size_t)NEN + 1)),
      *xn = malloc(sizeof(int) * ((size_t)NEN + 1));
  int *f1 = malloc(sizeof(int) * ((size_t)NEF + 1)), *f2 = malloc(sizeof(int) * ((size_t)NEF + 1)),
      *xf = malloc(sizeof(int) * ((size_t)NEF + 1));
  int64_t *ptmp = NULL;
  int ok = 1;
  const char *why = "";

  /* Step 0 (:1004-1014): group 0's faces into the face intvalues */
  for (int64_t k = foff[0]; k < foff[1]; k++) ivf[face2[k]] = face1[k];
  /* group 0 is the merged mesh: its points and tets stay where they are */
  int64_t np = poff[1], ne = toff[1];
  for (int64_t k = 1; k <= np; k++) {
    tmp[k - 1] = (int)k;
    pg[k - 1] = 0;
    po[k - 1] = (int)k;
  }
  for (int64_t k = 1; k <= ne; k++) {
    for (int l = 0; l < 4; l++) mv[4 * (k - 1) + l] = tet[4 * (k - 1) + l];
    mg[k - 1] = 0;
    mo[k - 1] = (int)k;
    flag[k - 1] = (int)k;
  }
  /* Step 1 (:452-459): group 0's nodes into the node intvalues */
  for (int64_t k = noff[0]; k < noff[1]; k++) ivn[node2[k]] = node1[k];
  /* Step 1, continued (:463-466, :335-403): the interface points of the other groups */
  for (int g = 1; g < ngrp; g++) {
    int *tmpJ = tmp + poff[g];
    for (int64_t k = noff[g]; k < noff[g + 1]; k++) {
      const int glo = node2[k], ip = node1[k];
      if (tmpJ[ip - 1]) continue;
      if (!ivn[glo]) {
        np++;                                   /* MMG3D_newPt on a packed mesh */
        tmpJ[ip - 1] = (int)np;
        ivn[glo] = (int)np;
        pg[np - 1] = g;
        po[np - 1] = ip;
      } else {
        tmpJ[ip - 1] = abs(ivn[glo]);
        ivn[glo] *= -1;
      }
    }
  }
  for (int g = 1; g < ngrp; g++) {
    int *tmpJ = tmp + poff[g], *flagJ = flag + toff[g];
    char *baseJ = base + toff[g];
    const int *tetJ = tet + 4 * toff[g];
    const int64_t npJ = poff[g + 1] - poff[g], neJ = toff[g + 1] - toff[g];
    /* Step 2 (:505-552): the points no entry has placed */
    for (int64_t k = 1; k <= npJ; k++) {
      if (tmpJ[k - 1]) continue;
      np++;
      tmpJ[k - 1] = (int)np;
      pg[np - 1] = g;
      po[np - 1] = (int)k;
    }
    /* Step 3 (:607-679): the interface tets, in the order of the face entries */
    for (int64_t k = foff[g]; k < foff[g + 1]; k++) {
      const int glo = face2[k];
      const int iel = face1[k] / 12, ifac = (face1[k] % 12) / 3, iploc = (face1[k] % 12) % 3;
      if (baseJ[iel - 1]) {
        if (!ivf[glo]) ivf[glo] = 12 * flagJ[iel - 1] + 3 * ifac + iploc;
        else ivf[glo] *= -1;
        continue;
      }
      baseJ[iel - 1] = 1;
      ne++;                                     /* MMG3D_newElt on a packed mesh */
      for (int l = 0; l < 4; l++) mv[4 * (ne - 1) + l] = tmpJ[tetJ[4 * (iel - 1) + l] - 1];
      mg[ne - 1] = g;
      mo[ne - 1] = iel;
      flagJ[iel - 1] = (int)ne;
      if (!ivf[glo]) ivf[glo] = 12 * (int)ne + 3 * ifac + iploc;
      else ivf[glo] *= -1;
    }
    /* Step 4 (:707-748): the other tets */
    for (int64_t k = 1; k <= neJ; k++) {
      if (baseJ[k - 1]) continue;
      baseJ[k - 1] = 1;
      ne++;
      for (int l = 0; l < 4; l++) mv[4 * (ne - 1) + l] = tmpJ[tetJ[4 * (k - 1) + l] - 1];
      mg[ne - 1] = g;
      mo[ne - 1] = (int)k;
      flagJ[k - 1] = (int)ne;
    }
  }
  /* Step 5, nodes (:783-852) */
  ptmp = malloc(sizeof(int64_t) * ((size_t)np + 1));
  for (int64_t k = 1; k <= np; k++) ptmp[k] = -1;
  int64_t poi_id_int = 0;
  for (int k = 0; k < next_node && ok; k++) {
    int64_t poi_id_glo = 0;
    const int64_t nitem = node_off[k + 1] - node_off[k];
    int *items = xn + node_off[k];
    for (int64_t i = 0; i < nitem; i++) {
      const int ip = abs(ivn[node_items[node_off[k] + i]]);
      if (!ip) { ok = 0; why = "an external node item names a slot nothing filled"; break; }
      if (ptmp[ip] < 0) {
        n1[poi_id_int] = ip;
        n2[poi_id_int] = (int)poi_id_int;
        items[poi_id_glo++] = (int)poi_id_int;
        ptmp[ip] = poi_id_int + (int64_t)k * np;
        poi_id_int++;
      } else if (ptmp[ip] < (int64_t)k * np) {
        items[poi_id_glo++] = (int)(ptmp[ip] % np);
      }
    }
    if (ok && poi_id_glo != nitem) { ok = 0; why = "a merged point appears twice in an external node communicator"; }
  }
  /* Step 5, faces (:885-932) */
  int64_t face_id_int = 0;
  for (int k = 0; k < next_face && ok; k++)
    for (int64_t i = face_off[k]; i < face_off[k + 1]; i++) {
      const int iel = abs(ivf[face_items[i]]);
      if (!iel) { ok = 0; why = "an external face item names a slot nothing filled"; break; }
      f1[face_id_int] = iel;
      f2[face_id_int] = (int)face_id_int;
      xf[i] = (int)face_id_int;
      face_id_int++;
    }
  if (ok && np >= 2147483647LL) { ok = 0; why = "merged np >= 2^31 - 1"; }

  if (ok) {
    if (sizes) { sizes->np = np; sizes->ne = ne; sizes->nnode = poi_id_int; sizes->nface = face_id_int; }
    if (tetra_v) memcpy(tetra_v, mv, sizeof(int) * 4 * (size_t)ne);
    if (tet_group) memcpy(tet_group, mg, sizeof(int) * (size_t)ne);
    if (tet_old) memcpy(tet_old, mo, sizeof(int) * (size_t)ne);
    if (point_group) memcpy(point_group, pg, sizeof(int) * (size_t)np);
    if (point_old) memcpy(point_old, po, sizeof(int) * (size_t)np);
    if (point_new) memcpy(point_new, tmp, sizeof(int) * (size_t)P);
    if (tet_new) memcpy(tet_new, flag, sizeof(int) * (size_t)T);
    if (out_node1) memcpy(out_node1, n1, sizeof(int) * (size_t)poi_id_int);
    if (out_node2) memcpy(out_node2, n2, sizeof(int) * (size_t)poi_id_int);
    if (out_face1) memcpy(out_face1, f1, sizeof(int) * (size_t)face_id_int);
    if (out_face2) memcpy(out_face2, f2, sizeof(int) * (size_t)face_id_int);
    if (ext_node_new) memcpy(ext_node_new, xn, sizeof(int) * (size_t)NEN);
    if (ext_face_new) memcpy(ext_face_new, xf, sizeof(int) * (size_t)NEF);
  }
  free(ivn); free(ivf); free(tmp); free(flag); free(base); free(mv); free(mg); free(mo); free(pg); free(po);
  free(n1); free(n2); free(xn); free(f1); free(f2); free(xf); free(ptmp);
  return ok ? 1 : refuse(why);
}
