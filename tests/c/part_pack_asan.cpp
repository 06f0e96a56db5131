// part_pack_asan.cpp -- the host step of pmx_part_from_marks under the DISTR
// target (parmmg_amd/csrc/pmx_part_pack.h: the used colours numbered from 0,
// ranks visited from myrank round) against the CPU twin's mir_part
// (tests/c/moveifc_ref.c), on random used[] tables for nprocs 1..5 and every
// myrank.  Stand-alone, built with -fsanitize=address,undefined by
// tests/test_part_cpu.py.  Prints "part pack asan ok".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pmx_part_pack.h"

extern "C" int mir_part(int64_t ne, const int *mark, int nprocs, int myrank, int nold_grp, int target,
                        const int *ngrps, int *part, int *ngrp);

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {          // xorshift64*, in 0..n-1
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (unsigned)(((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n);
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

int main() {
  long cases = 0;
  for (int nprocs = 1; nprocs <= 5; nprocs++)
    for (int myrank = 0; myrank < nprocs; myrank++)
      for (int rep = 0; rep < 200; rep++) {
        std::vector<int> ngrps((size_t)nprocs);
        std::vector<int64_t> sum((size_t)nprocs + 1, 0);
        for (int r = 0; r < nprocs; r++) {
          ngrps[(size_t)r] = (int)rnd(rep % 4 == 0 ? 40 : 5);     // 0 groups on a rank included
          sum[(size_t)r + 1] = sum[(size_t)r] + ngrps[(size_t)r];
        }
        const int64_t ntab = sum[(size_t)nprocs];
        const unsigned density = 1 + rnd(4);                      // a colour is used with probability density / 4
        std::vector<unsigned char> used((size_t)ntab, 0);
        std::vector<int> colours;
        for (int64_t c = 0; c < ntab; c++)
          if (rnd(4) < density) {
            used[(size_t)c] = 1;
            colours.push_back((int)c);
          }
        // the tets: every used colour at least once, in random order, as marks
        std::vector<int> mark(1, 0), col(1, 0);
        const size_t ne = colours.empty() ? 0 : colours.size() + rnd(3 * (unsigned)colours.size());
        for (size_t k = 0; k < ne; k++) {
          const int c = k < colours.size() ? colours[k] : colours[rnd((unsigned)colours.size())];
          int r = 0;
          while (c >= sum[(size_t)r + 1]) r++;
          col.push_back(c);
          mark.push_back((int)(c - sum[(size_t)r]) * nprocs + r);
        }
        for (size_t k = ne; k > 1; k--) {
          const size_t j = 1 + rnd((unsigned)k);
          std::swap(mark[k], mark[j]);
          std::swap(col[k], col[j]);
        }
        std::vector<int> part(ne + 1, -1), map((size_t)ntab + 1, -7), gm((size_t)ntab + 1, -7);
        int ngrp = -1;
        if (!mir_part((int64_t)ne, mark.data(), nprocs, myrank, ngrps[(size_t)myrank], 1, ngrps.data(), part.data(), &ngrp))
          FAIL("mir_part refused");
        const int count = pmx_part_pack_map(nprocs, myrank, sum.data(), used.data(), map.data(), gm.data());
        if (count != ngrp || count != (int)colours.size()) FAIL("count %d, the twin's %d", count, ngrp);
        if (map[(size_t)ntab] != -7 || gm[(size_t)count] != -7) FAIL("a write past the tables");
        for (int64_t c = 0; c < ntab; c++)
          if ((map[(size_t)c] >= 0) != (used[(size_t)c] != 0) || map[(size_t)c] >= count) FAIL("map of colour %lld", (long long)c);
        for (size_t k = 1; k <= ne; k++) {
          if (map[(size_t)col[k]] != part[k - 1]) FAIL("tet %zu: group %d, the twin's %d", k, map[(size_t)col[k]], part[k - 1]);
          if (gm[(size_t)part[k - 1]] != mark[k]) FAIL("tet %zu: group_mark %d, mark %d", k, gm[(size_t)part[k - 1]], mark[k]);
        }
        // group_mark is the inverse of the pack map
        for (int g = 0; g < count; g++) {
          const int r = gm[(size_t)g] % nprocs, q = gm[(size_t)g] / nprocs;
          if (map[(size_t)(sum[(size_t)r] + q)] != g) FAIL("group %d is not the map of its mark", g);
        }
        cases++;
      }
  printf("part pack asan ok (%ld tables)\n", cases);
  return 0;
}
