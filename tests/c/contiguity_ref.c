/* contiguity_ref.c -- the CPU twin of pmx_contiguity / pmx_fix_contiguity
 * (test infrastructure, one core).  Written from the semantics of DESIGN.md
 * section 4 ("Partition contiguity"), which restate ParMmg's
 * PMMG_check_grps_contiguity / PMMG_check_part_contiguity
 * (src/metis_pmmg.c:312-392,446-529) and PMMG_fix_contiguity*
 * (src/moveinterfaces_pmmg.c:148-299,377-523).  UNPINNED: Mmg is absent, so
 * the reference file cannot be built here and nothing ties this text to it
 * but the reading.
 *
 * adja is Mmg's: the neighbour of tet k (1-based) through face l is
 * adja[4 (k - 1) + 1 + l] / 4, 0 = none.  mark / flag / label arrays have
 * ne + 1 entries, slot 0 unused. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NB(adja, k, l) ((adja)[4 * ((int64_t)(k) - 1) + 1 + (l)] / 4)
#define UNSET 0

typedef struct {
  int64_t ncomp, nmerged, nmerged_tets, ncannot, counter;
} cgr_stats;

/* ---- breadth-first components ------------------------------------------ */

/* label[k] = the smallest tet of k's component in the graph restricted to
 * equal marks (mark NULL: one colour); returns the number of components.
 * counts (nparts entries, may be NULL): components per mark in 0..nparts-1. */
int64_t cgr_components(int64_t ne, const int *adja, const int *mark, int nparts, int *counts, int *label) {
  int *queue = (int *)malloc(sizeof(int) * (size_t)(ne + 1));
  int64_t ncomp = 0;
  memset(label, 0, sizeof(int) * (size_t)(ne + 1));
  if (counts) memset(counts, 0, sizeof(int) * (size_t)nparts);
  for (int64_t s = 1; s <= ne; s++) {
    if (label[s]) continue;
    const int c = mark ? mark[s] : 0;
    int64_t head = 0, tail = 0;
    label[s] = (int)s;
    queue[tail++] = (int)s;
    while (head < tail) {
      const int k = queue[head++];
      for (int l = 0; l < 4; l++) {
        const int k1 = NB(adja, k, l);
        if (!k1 || label[k1] || (mark && mark[k1] != c)) continue;
        label[k1] = (int)s;
        queue[tail++] = k1;
      }
    }
    ncomp++;
    if (counts && c >= 0 && c < nparts) counts[c]++;
  }
  free(queue);
  return ncomp;
}

/* ---- the two sweep counters -------------------------------------------- */

/* The whole-group counter: seed the first unseen tet with a new colour, then
 * sweep the tets from the seed upwards, giving the colour to every unseen
 * neighbour of a tet that has it, until a sweep changes nothing; again from
 * the top while tets are unseen.  Returns the number of colours used. */
int cgr_sweep_group(int64_t ne, const int *adja) {
  int *flag = (int *)calloc((size_t)(ne + 1), sizeof(int));
  int ncolors = 0;
  int64_t seen = 0;
  while (seen < ne) {
    int64_t istart = 0;
    int done = 1;
    for (int64_t ie = 1; ie <= ne; ie++)
      if (!flag[ie]) {
        flag[ie] = ++ncolors;
        seen++;
        istart = ie;
        done = 0;
        break;
      }
    while (!done) {
      done = 1;
      for (int64_t ie = istart; ie <= ne; ie++) {
        if (flag[ie] != ncolors) continue;
        for (int l = 0; l < 4; l++) {
          const int je = NB(adja, ie, l);
          if (je && !flag[je]) {
            flag[je] = ncolors;
            seen++;
            done = 0;
          }
        }
      }
    }
  }
  free(flag);
  return ncolors;
}

/* The per-part counter on the Metis graph (xadj / adjncy, 0-based nodes): the
 * same sweeps inside each part ipart = 0..nparts-1 in turn.  counts[ipart] =
 * that part's colours; returns the last part's, as the reference does. */
int cgr_sweep_parts(int64_t nnodes, const int *xadj, const int *adjncy, const int *part, int nparts, int *counts) {
  int *flag = (int *)calloc((size_t)(nnodes > 0 ? nnodes : 1), sizeof(int));
  int ncolors = 0;
  for (int ipart = 0; ipart < nparts; ipart++) {
    int64_t npart = 0, seen = 0;
    for (int64_t i = 0; i < nnodes; i++)
      if (part[i] == ipart) {
        flag[i] = 0;
        npart++;
      }
    ncolors = 0;
    while (seen < npart) {
      int64_t istart = 0;
      int done = 1;
      for (int64_t i = 0; i < nnodes; i++) {
        if (part[i] != ipart || flag[i]) continue;
        flag[i] = ++ncolors;
        seen++;
        istart = i;
        done = 0;
        break;
      }
      while (!done) {
        done = 1;
        for (int64_t i = istart; i < nnodes; i++) {
          if (part[i] != ipart || flag[i] != ncolors) continue;
          for (int a = xadj[i]; a < xadj[i + 1]; a++) {
            const int j = adjncy[a];
            if (part[j] != ipart || flag[j]) continue;
            flag[j] = ncolors;
            seen++;
            done = 0;
          }
        }
      }
    }
    if (counts) counts[ipart] = ncolors;
  }
  free(flag);
  return ncolors;
}

/* ---- FIX ---------------------------------------------------------------- */

typedef struct {
  int *tet;       /* the list, in enqueue order */
  int64_t len;
  int otetra;     /* UNSET: no neighbour outside the list */
} cgr_list;

typedef struct {
  int64_t ne;
  const int *adja;
  int *mark, *flag;
  int base;
} cgr_state;

/* LIST(start) into L (L->tet holds ne entries) */
static void cgr_make_list(cgr_state *S, int start, cgr_list *L) {
  const int c = S->mark[start];
  S->base++;
  S->flag[start] = S->base;
  L->len = 0;
  L->tet[L->len++] = start;
  for (int64_t cur = 0; cur < L->len; cur++) {
    const int k = L->tet[cur];
    for (int l = 0; l < 4; l++) {
      const int k1 = NB(S->adja, k, l);
      if (!k1) continue;
      if (S->flag[k1]) continue;
      if (S->mark[k1] != c) continue;
      S->flag[k1] = S->base;
      L->tet[L->len++] = k1;
    }
  }
  L->otetra = UNSET;
  for (int64_t cur = 0; cur < L->len && L->otetra == UNSET; cur++) {
    const int k = L->tet[cur];
    for (int l = 0; l < 4; l++) {
      const int k1 = NB(S->adja, k, l);
      if (k1 && S->flag[k1] != S->base) {
        L->otetra = k1;
        break;
      }
    }
  }
}

/* MERGE(list, otetra); returns flag[otetra] as read at merge time */
static int cgr_merge(cgr_state *S, const cgr_list *L) {
  const int m = S->mark[L->otetra], f = S->flag[L->otetra];
  for (int64_t i = 0; i < L->len; i++) {
    S->mark[L->tet[i]] = m;
    S->flag[L->tet[i]] = f;
  }
  return f;
}

/* FIX on mark[1..ne] (in/out) with the colours colors[0..ncolors-1] in that
 * order.  st->ncomp is left alone (the caller counts before the fix). */
void cgr_fix(int64_t ne, const int *adja, int *mark, int ncolors, const int *colors, cgr_stats *st) {
  cgr_state S = {ne, adja, mark, (int *)calloc((size_t)(ne + 1), sizeof(int)), 0};
  cgr_list A = {(int *)malloc(sizeof(int) * (size_t)(ne + 1)), 0, UNSET};
  cgr_list B = {(int *)malloc(sizeof(int) * (size_t)(ne + 1)), 0, UNSET};
  cgr_list *mainl = &A, *next = &B;
  int64_t counter = 0;
  st->nmerged = st->nmerged_tets = st->ncannot = 0;
  for (int ic = 0; ic < ncolors; ic++) {
    const int c = colors[ic];
    int64_t start = 1;
    while (start <= ne && mark[start] != c) start++;
    if (start > ne) continue;
    cgr_make_list(&S, (int)start, mainl);
    counter += mainl->len;
    for (;;) {
      start++;
      while (start <= ne && !(S.flag[start] == 0 && mark[start] == c)) start++;
      if (start > ne) break;
      cgr_make_list(&S, (int)start, next);
      counter += next->len;
      if (next->len > mainl->len) {
        if (mainl->otetra == UNSET) {
          st->ncannot++;
        } else {
          if (cgr_merge(&S, mainl) == 0) counter -= mainl->len;
          st->nmerged++;
          st->nmerged_tets += mainl->len;
          cgr_list *t = mainl;
          mainl = next;
          next = t;
        }
      } else {
        if (next->otetra == UNSET) {
          st->ncannot++;
        } else {
          if (cgr_merge(&S, next) == 0) counter -= next->len;
          st->nmerged++;
          st->nmerged_tets += next->len;
        }
      }
    }
  }
  st->counter = counter;
  free(S.flag);
  free(A.tet);
  free(B.tet);
}
