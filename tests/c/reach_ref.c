/* reach_ref.c -- the CPU twin of pmx_check_reachability and of the in-place
 * pmx_moveifc_fix / pmx_moveifc_reach (test infrastructure, one core).
 * Written from the semantics of DESIGN.md section 4 ("Reachability"), which
 * restate ParMmg's PMMG_list_contiguousColor, PMMG_merge_subgroup,
 * PMMG_fix_contiguity and steps 2-3 of PMMG_check_reachability
 * (src/moveinterfaces_pmmg.c:148-299, 377-523, 627-811).  UNPINNED: Mmg is
 * absent, so the reference file cannot be built here and nothing ties this
 * text to it but the reading.
 *
 * One state serves both calls, as in the reference: the tets' mark and flag
 * and the running base.  A list writes a fresh base into the flag of its tets;
 * a merged list takes its target's mark and flag.  The check therefore starts
 * from exactly the flags the fix left.
 *
 * adja is Mmg's: the neighbour of tet k (1-based) through face l is
 * adja[4 (k - 1) + 1 + l] / 4, 0 = none.  mark and flag have ne + 1 entries,
 * slot 0 unused. */
#include <stdint.h>
#include <stdlib.h>

typedef struct {
  int64_t nseeds, nreached, nreached_tets;
  int64_t nunreached, nmerged, nmerged_tets;
  int64_t nrescanned, ncannot, counter;
  int64_t fix_nmerged, fix_nmerged_tets, fix_ncannot;
  /* of the twin alone, to tell what a test case exercises: step-3 lists whose
   * target lay, flagged, in a list met earlier in step 3; step-3 lists that
   * hold a tet met before (a merge unflagged it) and lie beside a tet of their
   * own mark that step 2 flagged */
  int64_t nchained, nbeside_reached;
} rcr_stats;

typedef struct {
  int64_t ne;
  const int *adja;
  int *mark, *flag;
  int *base;
  int *list;      /* ne entries */
  int64_t len;
  int other;      /* the first neighbour outside the list in list order, 0: none */
} rcr_walk;

static int rcr_nb(const rcr_walk *W, int k, int l) { return W->adja[4 * ((int64_t)k - 1) + 1 + l] / 4; }

/* the unflagged tets of start's mark reachable from start through faces,
 * breadth-first, faces 0..3; every one takes the new base */
static void rcr_list(rcr_walk *W, int start) {
  const int colour = W->mark[start];
  const int b = ++*W->base;
  int64_t head = 0;
  W->len = 0;
  W->list[W->len++] = start;
  W->flag[start] = b;
  while (head < W->len) {
    const int k = W->list[head++];
    for (int l = 0; l < 4; l++) {
      const int k1 = rcr_nb(W, k, l);
      if (k1 == 0 || W->flag[k1] != 0 || W->mark[k1] != colour) continue;
      W->flag[k1] = b;
      W->list[W->len++] = k1;
    }
  }
  W->other = 0;
  for (int64_t i = 0; i < W->len && !W->other; i++)
    for (int l = 0; l < 4 && !W->other; l++) {
      const int k1 = rcr_nb(W, W->list[i], l);
      if (k1 != 0 && W->flag[k1] != b) W->other = k1;
    }
}

/* the list joins its target; returns the flag it took */
static int rcr_join(rcr_walk *W, const int *list, int64_t len, int other) {
  const int m = W->mark[other], f = W->flag[other];
  for (int64_t i = 0; i < len; i++) {
    W->mark[list[i]] = m;
    W->flag[list[i]] = f;
  }
  return f;
}

/* PMMG_fix_contiguity: flag is zeroed, *base goes on from its value; for
 * every colour in order, the largest list met so far stays ("main"), every
 * other one joins its first outside neighbour.  st: fix_* and counter. */
void rcr_fix(int64_t ne, const int *adja, int *mark, int *flag, int *base, int ncolors, const int *colors,
             rcr_stats *st) {
  int *keep = (int *)malloc(sizeof(int) * (size_t)(ne + 1));
  int *scratch = (int *)malloc(sizeof(int) * (size_t)(ne + 1));
  rcr_walk W = {ne, adja, mark, flag, base, scratch, 0, 0};
  int64_t counter = 0;
  st->fix_nmerged = st->fix_nmerged_tets = st->fix_ncannot = 0;
  for (int64_t k = 0; k <= ne; k++) flag[k] = 0;
  for (int ic = 0; ic < ncolors; ic++) {
    const int c = colors[ic];
    int64_t at = 1;
    while (at <= ne && mark[at] != c) at++;
    if (at > ne) continue;
    /* the main list lives in `keep`, the candidate in `scratch` */
    W.list = keep;
    rcr_list(&W, (int)at);
    int64_t main_len = W.len;
    int main_other = W.other;
    counter += main_len;
    for (at++; at <= ne; at++) {
      if (flag[at] != 0 || mark[at] != c) continue;
      W.list = scratch;
      rcr_list(&W, (int)at);
      counter += W.len;
      const int cand_bigger = W.len > main_len;
      const int *lose = cand_bigger ? keep : scratch;
      const int64_t lose_len = cand_bigger ? main_len : W.len;
      const int lose_other = cand_bigger ? main_other : W.other;
      if (lose_other == 0) {
        st->fix_ncannot++;      /* nothing moves: a main without a way out stays main */
        continue;
      }
      if (rcr_join(&W, lose, lose_len, lose_other) == 0) counter -= lose_len;
      st->fix_nmerged++;
      st->fix_nmerged_tets += lose_len;
      if (cand_bigger) {
        int *t = keep;
        keep = scratch;
        scratch = t;
        main_len = W.len;
        main_other = W.other;
      }
    }
  }
  st->counter = counter;
  free(keep);
  free(scratch);
}

/* Steps 2 and 3 of PMMG_check_reachability on the state a fix left.
 * color_in[i]: the colour received for entry i after the discard, -1 = none.
 * st->counter: in, the fix's; out, the reference's.  Returns 0 when an entry's
 * tet lies outside 1..ne (nothing touched). */
int rcr_reach(int64_t ne, const int *adja, int *mark, int *flag, int *base, int64_t nface, const int *face_index1,
              const int *color_in, rcr_stats *st) {
  for (int64_t i = 0; i < nface; i++)
    if (face_index1[i] / 12 < 1 || face_index1[i] / 12 > ne) return 0;
  int *list = (int *)malloc(sizeof(int) * (size_t)(ne + 1));
  rcr_walk W = {ne, adja, mark, flag, base, list, 0, 0};
  int64_t counter = st->counter;
  const int base0 = *base;      /* a flag above it was written by step 2 */
  char *met = (char *)calloc((size_t)(ne + 1), 1);
  st->nseeds = st->nreached = st->nreached_tets = 0;
  st->nunreached = st->nmerged = st->nmerged_tets = st->nrescanned = st->ncannot = 0;
  st->nchained = st->nbeside_reached = 0;
  /* step 2: every entry whose tet has the colour its neighbour reports */
  for (int64_t i = 0; i < nface; i++) {
    const int ie = face_index1[i] / 12, c = color_in[i];
    if (c == -1 || mark[ie] != c) continue;
    if (flag[ie] == 0 || flag[ie] > base0) st->nseeds++;   /* unflagged on entry */
    if (flag[ie] != 0) continue;
    rcr_list(&W, ie);
    counter += W.len;
    st->nreached++;
    st->nreached_tets += W.len;
  }
  /* step 3: what no entry reached joins a neighbour */
  const int base2 = *base;
  for (int64_t ie = 1; ie <= ne; ie++) {
    if (flag[ie] != 0) continue;
    rcr_list(&W, (int)ie);
    counter += W.len;
    st->nunreached++;
    int beside = 0, again = 0;
    for (int64_t i = 0; i < W.len; i++) {
      again |= met[W.list[i]];
      for (int l = 0; l < 4; l++) {
        const int k1 = rcr_nb(&W, W.list[i], l);
        if (k1 && flag[k1] > base0 && flag[k1] <= base2 && mark[k1] == mark[ie]) beside = 1;
      }
    }
    st->nbeside_reached += beside && again;
    if (W.other && met[W.other] && flag[W.other] != 0) st->nchained++;
    for (int64_t i = 0; i < W.len; i++) met[W.list[i]] = 1;
    if (W.other == 0) {
      st->ncannot++;
      continue;
    }
    st->nmerged++;
    st->nmerged_tets += W.len;
    if (rcr_join(&W, W.list, W.len, W.other) == 0) {
      counter -= W.len;        /* unflagged again under the new colour: met again further on */
      st->nrescanned++;
    }
  }
  st->counter = counter;
  free(list);
  free(met);
  return 1;
}
