/* moveifc_ref.c -- the CPU twin of pmx_moveifc_* (test infrastructure, one
 * core).  Written from the semantics of DESIGN.md section 4 ("Interface
 * displacement"), which restate ParMmg's PMMG_set_color_tetra,
 * PMMG_mark_interfacePoints, PMMG_mark_boulevolp, PMMG_mark_sideFront,
 * PMMG_part_moveInterfaces and PMMG_part_getInterfaces
 * (src/moveinterfaces_pmmg.c:119-134, 832-1090, 1150-1212, 1306-1440): the
 * sequential loops in the reference's order, with its base / flag counters,
 * negrp / nemin, the two block checks and the ball overflow.  UNPINNED: Mmg is
 * absent, so the reference file cannot be built here and nothing ties this
 * text to it but the reading.
 *
 * tet is Mmg's connectivity (row k = tet k, row 0 unused), adja Mmg's
 * adjacency: the neighbour of tet k through face l is adja[4 (k - 1) + 1 + l]
 * / 4, 0 = none.  mark has ne + 1 entries, tmp / s / flag np + 1, slot 0
 * unused.  Between layers flag is 1 on the front and 0 elsewhere; inside a
 * layer 2 = touched (the reference's base_front + 1) and 3 = next
 * (base_front + 2). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NB(adja, k, l) ((adja)[4 * ((int64_t)(k) - 1) + 1 + (l)] / 4)
#define UNSET (-1)
#define LMAX 10240            /* MMG3D_LMAX */
#define NELEM_MIN 6           /* PMMG_REDISTR_NELEM_MIN */

static const int inxt3[7] = {1, 2, 3, 0, 1, 2, 3};

/* the priority map: nprocs, myrank, the old groups of this rank, displsgrp
 * (nprocs + 1 entries) and mapgrp (displsgrp[nprocs] entries) */
typedef struct {
  int nprocs, myrank, nold_grp;
  const int *displsgrp, *mapgrp;
} mir_map;

/* front: front points the layer walked; touched / next: points the layer
 * left touched / next (together the following front); recolor: tet
 * recolourings (a tet that changes twice counts twice); blocks: balls
 * abandoned at nemin; maxball: the longest ball walked to its end;
 * overflow_ip: the point whose ball overflowed (0: none) */
typedef struct {
  int64_t front, touched, recolor, next, blocks, maxball, overflow_ip;
} mir_stats;

static int weight(const mir_map *m, int c) { return m->mapgrp[c / m->nprocs + m->displsgrp[c % m->nprocs]]; }
/* PMMG_get_ifcDirection(c0, c1): c1 beats c0 */
static int beats(const mir_map *m, int c0, int c1) { return weight(m, c0) > weight(m, c1); }

/* PMMG_set_color_tetra per old group, PMMG_mark_interfacePoints and the
 * negrp / nemin of PMMG_part_moveInterfaces; returns the front points */
int64_t mir_begin(int64_t ne, int64_t np, const int *tet, const mir_map *m, const int *tet_group, int *mark, int *tmp,
                  int *s, int *flag, int *negrp, int *nemin) {
  int64_t nfront = 0;
  mark[0] = 0;
  for (int64_t k = 1; k <= ne; k++) mark[k] = m->nprocs * tet_group[k - 1] + m->myrank;
  for (int64_t p = 0; p <= np; p++) {
    tmp[p] = UNSET;
    s[p] = UNSET;
    flag[p] = 0;
  }
  for (int64_t k = 1; k <= ne; k++)
    for (int iloc = 0; iloc < 4; iloc++) {
      const int p = tet[4 * k + iloc];
      if (tmp[p] == UNSET) {
        tmp[p] = mark[k];
        s[p] = (int)(4 * k + iloc);
        continue;
      }
      if (beats(m, tmp[p], mark[k])) {
        tmp[p] = mark[k];
        s[p] = (int)(4 * k + iloc);
        flag[p] = 1;
      }
    }
  for (int64_t p = 1; p <= np; p++) nfront += flag[p];
  for (int g = 0; g < m->nold_grp; g++) {
    negrp[g] = m->mapgrp[g + m->displsgrp[m->myrank]];
    nemin[g] = negrp[g] / 2 + 1 < NELEM_MIN ? negrp[g] / 2 + 1 : NELEM_MIN;
  }
  return nfront;
}

/* the receiving end of the node-communicator exchange: the listed points take
 * the reduced colours and join the front, whether their colour changed or not */
void mir_set_colors(int64_t n, const int *ip, const int *color, int *tmp, int *flag) {
  for (int64_t i = 0; i < n; i++) {
    tmp[ip[i]] = color[i];
    flag[ip[i]] = 1;
  }
}

typedef struct {
  int64_t ne, np;
  const int *tet, *adja;
  const mir_map *m;
  int *mark, *tmp, *s, *flag, *negrp, *nemin;
  int *tflag, base, *list;
  mir_stats *st;
} mir_ctx;

/* the three other vertices of tet k, recoloured with `color`, seen from local
 * vertex j1 */
static void spread(mir_ctx *c, int k, int j1, int color) {
  for (int j = 0; j < 3; j++) {
    const int j2 = inxt3[j1 + j], q = c->tet[4 * (int64_t)k + j2];
    if (c->flag[q] != 1 && c->flag[q] != 2) {
      if (beats(c->m, c->tmp[q], color)) {
        c->tmp[q] = color;
        c->s[q] = 4 * k + j2;
      }
      c->flag[q] = 3;
    } else
      c->flag[q] = 2;
  }
}

/* a recolouring of tet k by `color`: 0 when the tet's group is at nemin
 * (start: the <= check of the start tet) */
static int recolor(mir_ctx *c, int k, int j1, int color, int start) {
  const mir_map *m = c->m;
  const int old = c->mark[k];
  if (old % m->nprocs == m->myrank) {
    const int g = old / m->nprocs;
    if (start ? c->negrp[g] <= c->nemin[g] : c->negrp[g] == c->nemin[g]) return 0;
    c->negrp[g]--;
  }
  c->mark[k] = color;
  c->st->recolor++;
  spread(c, k, j1, color);
  return 1;
}

/* PMMG_mark_boulevolp: the ball's length, 1 after a block as the reference
 * returns, 0 on overflow */
static int ball_mark(mir_ctx *c, int ip) {
  const int start = c->s[ip] / 4, iloc = c->s[ip] % 4, color = c->tmp[ip];
  const int base = ++c->base;
  int ilist = 1, cur = 0;
  c->tflag[start] = base;
  c->list[0] = 4 * start + iloc;
  if (beats(c->m, c->mark[start], color) && !recolor(c, start, iloc, color, 1)) {
    c->st->blocks++;
    return 1;
  }
  while (cur < ilist) {
    const int k = c->list[cur] / 4;
    int i = c->list[cur] % 4;
    for (int l = 0; l < 3; l++) {
      int j1 = 0;
      i = inxt3[i];
      const int k1 = NB(c->adja, k, i);
      if (!k1 || c->tflag[k1] == base) continue;
      while (c->tet[4 * (int64_t)k1 + j1] != ip) j1++;
      if (beats(c->m, c->mark[k1], color) && !recolor(c, k1, j1, color, 0)) {
        c->st->blocks++;
        return 1;
      }
      c->tflag[k1] = base;
      if (ilist > LMAX - 3) return 0;
      c->list[ilist++] = 4 * k1 + j1;
    }
    cur++;
  }
  if (ilist > c->st->maxball) c->st->maxball = ilist;
  return ilist;
}

/* PMMG_mark_sideFront_ppt */
static int ball_side(mir_ctx *c, int ip) {
  const int start = c->s[ip] / 4, iloc = c->s[ip] % 4;
  const int base = ++c->base;
  int ilist = 1, cur = 0;
  c->tflag[start] = base;
  c->list[0] = 4 * start + iloc;
  if (beats(c->m, c->tmp[ip], c->mark[start])) c->tmp[ip] = c->mark[start];
  while (cur < ilist) {
    const int k = c->list[cur] / 4;
    int i = c->list[cur] % 4;
    for (int l = 0; l < 3; l++) {
      int j1 = 0;
      i = inxt3[i];
      const int k1 = NB(c->adja, k, i);
      if (!k1 || c->tflag[k1] == base) continue;
      while (c->tet[4 * (int64_t)k1 + j1] != ip) j1++;
      if (beats(c->m, c->tmp[ip], c->mark[k1])) {
        c->tmp[ip] = c->mark[k1];
        c->s[ip] = 4 * k1 + j1;
      }
      c->tflag[k1] = base;
      if (ilist > LMAX - 3) return 0;
      c->list[ilist++] = 4 * k1 + j1;
    }
    cur++;
  }
  if (ilist > c->st->maxball) c->st->maxball = ilist;
  return ilist;
}

/* One layer of PMMG_part_moveInterfaces after the exchange: the front points'
 * balls in ascending order, the side fronts, the next front.  Returns 0 on a
 * ball overflow: st->overflow_ip names the point and the arrays are left as
 * the reference leaves them, half-way through the layer.  A point in no tet
 * (s < 0) has no ball and is skipped. */
int mir_layer(int64_t ne, int64_t np, const int *tet, const int *adja, const mir_map *m, int *mark, int *tmp, int *s,
              int *flag, int *negrp, int *nemin, mir_stats *st) {
  mir_ctx c = {ne, np, tet, adja, m, mark, tmp, s, flag, negrp, nemin, NULL, 0, NULL, st};
  int ok = 1;
  memset(st, 0, sizeof *st);
  c.tflag = (int *)calloc((size_t)(ne + 1), sizeof(int));
  c.list = (int *)malloc(sizeof(int) * (LMAX + 2));
  for (int64_t ip = 1; ip <= np && ok; ip++) {
    if ((flag[ip] != 1 && flag[ip] != 2) || s[ip] < 0) continue;
    st->front++;
    if (!ball_mark(&c, (int)ip)) {
      st->overflow_ip = ip;
      ok = 0;
    }
  }
  for (int64_t ip = 1; ip <= np && ok; ip++) {
    if (flag[ip] != 2) continue;
    st->touched++;
    if (!ball_side(&c, (int)ip)) {
      st->overflow_ip = ip;
      ok = 0;
    }
    flag[ip] = 3;
  }
  if (ok)
    for (int64_t ip = 1; ip <= np; ip++) {
      flag[ip] = flag[ip] == 3;
      st->next += flag[ip];
    }
  free(c.tflag);
  free(c.list);
  return ok;
}

/* PMMG_part_getInterfaces: target 1 (PMMG_GRPSPL_DISTR_TARGET) the compacted
 * numbering over all ranks' groups, ranks visited from myrank round; target 2
 * (PMMG_GRPSPL_MMG_TARGET) the old group, 0 when a mark is foreign (the
 * reference asserts).  ngrps: the old groups of every rank.  Returns 1 and
 * the groups required in *ngrp. */
int mir_part(int64_t ne, const int *mark, int nprocs, int myrank, int nold_grp, int target, const int *ngrps, int *part,
             int *ngrp) {
  if (target == 2) {
    for (int64_t k = 1; k <= ne; k++)
      if (mark[k] % nprocs != myrank) return 0;
    for (int64_t k = 1; k <= ne; k++) part[k - 1] = mark[k] / nprocs;
    *ngrp = nold_grp;
    return 1;
  }
  int *sum = (int *)calloc((size_t)nprocs + 1, sizeof(int));
  for (int i = 0; i < nprocs; i++) sum[i + 1] = sum[i] + ngrps[i];
  int *map = (int *)calloc((size_t)sum[nprocs] + 1, sizeof(int));
  int count = 0;
  for (int64_t k = 1; k <= ne; k++) {
    part[k - 1] = mark[k] / nprocs + sum[mark[k] % nprocs];
    map[part[k - 1]] = 1;
  }
  for (int i = 0; i < nprocs; i++) {
    const int iproc = (i + myrank) % nprocs;
    for (int g = 0; g < ngrps[iproc]; g++)
      if (map[g + sum[iproc]]) map[g + sum[iproc]] = count++;
  }
  for (int64_t k = 1; k <= ne; k++) part[k - 1] = map[part[k - 1]];
  free(sum);
  free(map);
  *ngrp = count;
  return 1;
}
