/* split_ref.c -- CPU twin of pmx_split_groups / pmx_split_fetch (test
 * infrastructure).  A sequential restatement, on plain arrays, of the loops of
 * the reference's PMMG_split_eachGrp (src/grpsplit_pmmg.c:1267-1445):
 * PMMG_splitGrps_countTetPerGrp (:1106-1116), PMMG_splitGrps_fillGroup
 * (:819-1094) and the four communicator updates it calls (:606-795).  The
 * point fields the reference borrows are arrays here: tmp (the vertex's value
 * in the internal node communicator, -1 unset), s (the group that copied the
 * vertex last), flag (its local id there); MMG5_Tetra.flag is tet_new (old
 * mesh) and tet_old (new meshes).  xTetra / xPoint appends, tags and the mesh
 * cleaning are left out: they touch none of the arrays compared.
 *
 * UNPINNED: the reference file needs Mmg, which is absent, so this file is
 * checked by the properties of tests/test_split_cpu.py, not against a build
 * of the reference.
 *
 * Layout: tet[4*k + s], k = 1..ne (row 0 unused); adja[4*(k-1) + 1 + f] =
 * 4*k' + f' or 0 (Mmg); part[k-1] in 0..ngrp-1.  Outputs are the groups'
 * arrays one after the other in the order g = 0..ngrp-1: tet_old (ne),
 * tetra_v and adja_new (4 ints per local tet, face f at 4*(j-1) + f), point_old,
 * the face lists and the node lists (sizes[g] entries each). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int64_t ne, np, nface, nnode; } spr_sizes;

static const int idir[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};

/* returns 1, or 0 on an allocation failure / an empty part */
int spr_split(int64_t ne, int64_t np, const int *tet, const int *adja, const int *part, int ngrp,
              int64_t nface_in, const int *face_in1, const int *face_in2,
              int64_t nnode_in, const int *node_in1, const int *node_in2,
              int64_t *int_face_nitem, int64_t *int_node_nitem,
              spr_sizes *sizes, int *tet_new, int *tet_old, int *tetra_v, int *adja_new, int *point_old,
              int *face1, int *face2, int *node1, int *node2) {
  int *cnt = calloc((size_t)ngrp, sizeof(int)), *toff = calloc((size_t)ngrp + 1, sizeof(int));
  int *posIn = malloc(sizeof(int) * (size_t)(4 * ne + 1)), *iplocIn = malloc(sizeof(int) * (size_t)(4 * ne + 1));
  int *tmp = malloc(sizeof(int) * (size_t)(np + 1)), *s = malloc(sizeof(int) * (size_t)(np + 1));
  int *flag = malloc(sizeof(int) * (size_t)(np + 1));
  int *ctmp = malloc(sizeof(int) * (size_t)(np + 1));   /* tmp of the group's copies, by local id */
  int ok = cnt && toff && posIn && iplocIn && tmp && s && flag && ctmp;
  int64_t fnitem = *int_face_nitem, nnitem = *int_node_nitem;
  int64_t poff = 0, foff = 0, noff = 0;
  if (!ok) goto done;

  for (int64_t i = 0; i <= 4 * ne; i++) posIn[i] = iplocIn[i] = -1;
  for (int64_t i = 0; i < nface_in; i++) {
    const int ie = face_in1[i] / 12, fac = (face_in1[i] % 12) / 3;
    posIn[4 * (ie - 1) + 1 + fac] = face_in2[i];
    iplocIn[4 * (ie - 1) + 1 + fac] = (face_in1[i] % 12) % 3;
  }
  for (int64_t p = 1; p <= np; p++) tmp[p] = s[p] = -1;
  for (int64_t i = 0; i < nnode_in; i++) tmp[node_in1[i]] = node_in2[i];

  /* countTetPerGrp, and the old tet of every new tet */
  for (int64_t ie = 1; ie <= ne; ie++) tet_new[ie - 1] = ++cnt[part[ie - 1]];
  for (int g = 0; g < ngrp; g++) {
    toff[g + 1] = toff[g] + cnt[g];
    if (cnt[g] == 0) ok = 0;
  }
  if (!ok) goto done;
  for (int64_t ie = 1; ie <= ne; ie++) tet_old[toff[part[ie - 1]] + tet_new[ie - 1] - 1] = (int)ie;

  for (int g = 0; g < ngrp; g++) {
    const int neg = cnt[g];
    const int *told = tet_old + toff[g];
    int *tv = tetra_v + 4 * (int64_t)toff[g], *ad = adja_new + 4 * (int64_t)toff[g];
    int *pold = point_old + poff, *f1 = face1 + foff, *f2 = face2 + foff, *n1 = node1 + noff, *n2 = node2 + noff;
    int npg = 0, nf = 0, nn = 0;

    for (int j = 1; j <= neg; j++) {
      const int k = told[j - 1];
      const int *pv = tet + 4 * (int64_t)k;
      for (int poi = 0; poi < 4; poi++) {
        const int v = pv[poi];
        if (s[v] != g) {
          ++npg;
          pold[npg - 1] = v;
          ctmp[npg] = tmp[v];                 /* memcpy of the point */
          tv[4 * (j - 1) + poi] = npg;
          s[v] = g;
          flag[v] = npg;
          /* updateNodeCommOld */
          if (ctmp[npg] != -1) {
            n1[nn] = npg;
            n2[nn] = ctmp[npg];
            nn++;
            ++nnitem;
          }
        } else {
          tv[4 * (j - 1) + poi] = flag[v];
        }
      }
      int *a = ad + 4 * (j - 1);
      memcpy(a, adja + 4 * ((int64_t)k - 1) + 1, 4 * sizeof(int));
      for (int fac = 0; fac < 4; fac++) {
        /* updateFaceCommOld */
        const int64_t pos = 4 * ((int64_t)k - 1) + 1 + fac;
        if (a[fac] == 0) {
          if (posIn[pos] >= 0) {
            f1[nf] = 12 * j + 3 * fac + iplocIn[pos];
            f2[nf] = posIn[pos];
            nf++;
          }
          continue;
        }
        const int adjidx = a[fac] / 4, vidx = a[fac] % 4;
        if (part[adjidx - 1] != g) {
          a[fac] = 0;
          /* updateFaceCommNew */
          const int64_t apos = 4 * ((int64_t)adjidx - 1) + 1 + vidx;
          if (posIn[apos] < 0) {
            posIn[pos] = posIn[apos] = (int)fnitem;
            const int ip = pv[idir[fac][0]];
            int iplocadj;
            for (iplocadj = 0; iplocadj < 3; iplocadj++)
              if (tet[4 * (int64_t)adjidx + idir[vidx][iplocadj]] == ip) break;
            iplocIn[pos] = 0;
            iplocIn[apos] = iplocadj;
            f1[nf] = 12 * j + 3 * fac + 0;
            f2[nf] = posIn[pos];
            nf++;
            ++fnitem;
          } else {
            f1[nf] = 12 * j + 3 * fac + iplocIn[pos];
            f2[nf] = posIn[pos];
            nf++;
          }
        } else if (adjidx < k) {
          const int jn = tet_new[adjidx - 1];
          a[fac] = 4 * jn + vidx;
          ad[4 * (jn - 1) + vidx] = 4 * j + fac;
        }
      }
    }
    /* updateNodeCommNew over the group's tets */
    for (int j = 1; j <= neg; j++) {
      const int k = told[j - 1];
      const int *oa = adja + 4 * ((int64_t)k - 1) + 1;
      for (int fac = 0; fac < 4; fac++) {
        const int adjidx = oa[fac] / 4;
        if (!adjidx || part[adjidx - 1] == g) continue;
        for (int poi = 0; poi < 3; poi++) {
          const int lp = tv[4 * (j - 1) + idir[fac][poi]];
          if (ctmp[lp] == -1) {
            n1[nn] = lp;
            n2[nn] = (int)(nnitem + 1);
            nn++;
            tmp[tet[4 * (int64_t)k + idir[fac][poi]]] = (int)(nnitem + 1);
            ctmp[lp] = (int)(nnitem + 1);
            ++nnitem;
          }
        }
      }
    }
    sizes[g].ne = neg;
    sizes[g].np = npg;
    sizes[g].nface = nf;
    sizes[g].nnode = nn;
    poff += npg;
    foff += nf;
    noff += nn;
  }
  *int_face_nitem = fnitem;
  *int_node_nitem = nnitem;
done:
  free(cnt); free(toff); free(posIn); free(iplocIn); free(tmp); free(s); free(flag); free(ctmp);
  return ok;
}
