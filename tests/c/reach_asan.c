/* reach_asan.c -- the CPU twin of the reachability check (reach_ref.c) driven
 * end to end on generated cubes, for an ASan/UBSan build
 * (tests/test_reach_sanitizer.py): z-slabs of eight colours of which rank 1 of
 * 3 owns 1, 4 and 7, with pseudo-random fragments, the bottom boundary tets as
 * the entries towards rank 0 and the top ones towards rank 2, first with
 * honest colours, then with pseudo-random ones.  It checks what can be checked
 * without a second implementation: the flags after the fix say "local colour",
 * every tet ends flagged, the counter ends at ne, a local tet keeps its mark,
 * and an entry out of range is refused with nothing touched. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  int64_t nseeds, nreached, nreached_tets, nunreached, nmerged, nmerged_tets, nrescanned, ncannot, counter;
  int64_t fix_nmerged, fix_nmerged_tets, fix_ncannot, nchained, nbeside_reached;
} rcr_stats;
void rcr_fix(int64_t ne, const int *adja, int *mark, int *flag, int *base, int ncolors, const int *colors,
             rcr_stats *st);
int rcr_reach(int64_t ne, const int *adja, int *mark, int *flag, int *base, int64_t nface, const int *face_index1,
              const int *color_in, rcr_stats *st);
void pmg_kuhn_counts(int n, int64_t *np, int64_t *ne, int64_t *nt);
int64_t pmg_kuhn_cube(int n, uint64_t seed, double jitter, double *xyz, int *tet, int *adja, int *tria, int *adjt);

static int *ints(size_t n) { return calloc(n + 1, sizeof(int)); }

static void fail(const char *what) {
  fprintf(stderr, "reach asan: %s\n", what);
  exit(1);
}

static int local(int c) { return c == 1 || c == 4 || c == 7; }

/* kind 0: honest colours, 1: pseudo-random colours and marks */
static void run(int n, int kind) {
  int64_t np, ne, nt;
  pmg_kuhn_counts(n, &np, &ne, &nt);
  double *xyz = malloc(sizeof(double) * 3 * (size_t)(np + 1));
  int *tet = ints(4 * (size_t)(ne + 1)), *adja = ints((size_t)(4 * ne + 5));
  int *tria = ints(3 * (size_t)(nt + 1)), *adjt = ints((size_t)(3 * nt + 4));
  if (pmg_kuhn_cube(n, 20250117u, 0.15, xyz, tet, adja, tria, adjt) != nt) exit(2);
  int *mark = ints((size_t)ne + 1), *flag = ints((size_t)ne + 1), *fixed = ints((size_t)ne + 1);
  int *fi = ints((size_t)ne), *cin = ints((size_t)ne);
  const int colors[3] = {1, 4, 7}, slab[8] = {0, 0, 1, 4, 4, 7, 2, 2};
  uint64_t rng = 88172645463325252ull;
  int64_t nface = 0;
  for (int64_t k = 1; k <= ne; k++) {
    double z = 0;
    for (int j = 0; j < 4; j++) z += xyz[3 * (size_t)tet[4 * k + j] + 2] / 4;
    rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
    const int s = (int)(z * 8) > 7 ? 7 : (int)(z * 8);
    mark[k] = kind == 1 ? (int)(rng % 8) : (rng % 11 == 0 ? (int)((rng >> 8) % 9) : slab[s]);
    const int bdy = !adja[4 * (k - 1) + 1] || !adja[4 * (k - 1) + 2] || !adja[4 * (k - 1) + 3] || !adja[4 * (k - 1) + 4];
    if (bdy && (z * n < 1 || z * n > n - 1)) fi[nface++] = (int)(12 * k + 3);
  }
  int base = 0;
  rcr_stats st;
  memset(&st, 0, sizeof st);
  rcr_fix(ne, adja, mark, flag, &base, 3, colors, &st);
  int64_t nflag = 0;
  for (int64_t k = 1; k <= ne; k++) {
    if ((flag[k] != 0) != local(mark[k])) fail("a flag after the fix that does not say \"local colour\"");
    nflag += flag[k] != 0;
  }
  if (nflag != st.counter) fail("the fix's counter");
  memcpy(fixed, mark, sizeof(int) * (size_t)(ne + 1));
  for (int64_t i = 0; i < nface; i++) {
    const int ie = fi[i] / 12, c = mark[ie];
    double z = 0;
    for (int j = 0; j < 4; j++) z += xyz[3 * (size_t)tet[4 * ie + j] + 2] / 4;
    const int rank = z * n < 1 ? 0 : 2;
    rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
    cin[i] = kind == 1 ? (int)(rng % 10) - 1 : (c % 3 == rank ? c : -1);
  }
  int bad = (int)(12 * (ne + 1));
  const int64_t c0 = st.counter;
  if (rcr_reach(ne, adja, mark, flag, &base, 1, &bad, cin, &st)) fail("an entry out of range was taken");
  if (memcmp(fixed, mark, sizeof(int) * (size_t)(ne + 1)) || st.counter != c0) fail("a refusal touched the state");
  if (!rcr_reach(ne, adja, mark, flag, &base, nface, fi, cin, &st)) fail("the check refused its entries");
  for (int64_t k = 1; k <= ne; k++) {
    if (!flag[k]) fail("a tet left unflagged");
    if (local(fixed[k]) && mark[k] != fixed[k]) fail("a local tet changed its mark");
  }
  if (st.counter != ne) fail("the counter does not end at ne");
  if (st.nunreached != st.nmerged + st.ncannot) fail("lists met != merged + cannot");
  if (kind == 1 && !st.nrescanned) fail("the random case rescanned nothing");
  printf("n %d kind %d: %lld entries, %lld reached, %lld merged, %lld rescanned\n", n, kind, (long long)nface,
         (long long)st.nreached, (long long)st.nmerged, (long long)st.nrescanned);
  free(xyz), free(tet), free(adja), free(tria), free(adjt), free(mark), free(flag), free(fixed), free(fi), free(cin);
}

int main(void) {
  run(4, 0);
  run(6, 0);
  run(4, 1);
  run(6, 1);
  run(1, 1);
  printf("reach asan ok\n");
  return 0;
}
