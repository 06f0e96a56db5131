// pmx_part_pack.h -- the host step between the two passes of
// PMMG_part_getInterfaces under PMMG_GRPSPL_DISTR_TARGET (reference
// src/moveinterfaces_pmmg.c:1180-1207): the used colours numbered from 0, the
// ranks visited from myrank round.  Plain C++, no HIP: the library's
// pmx_part.hip and the stand-alone checker tests/c/part_pack_asan.cpp share it.
#pragma once
#include <cstdint>

// sum[r]: the colours before rank r's (nprocs + 1 entries, sum[0] = 0); a
// colour is c = mark / nprocs + sum[mark % nprocs].  used[c] != 0: a tet
// carries it.  map[c] receives the group of a used colour and -1 otherwise;
// group_mark[g] (may be null; as many entries as used colours) the mark every
// tet of group g carries.  Returns the number of groups.
inline int pmx_part_pack_map(int nprocs, int myrank, const int64_t *sum, const unsigned char *used, int *map,
                             int *group_mark) {
  int count = 0;
  for (int i = 0; i < nprocs; i++) {
    const int r = (i + myrank) % nprocs;
    for (int64_t c = sum[r]; c < sum[r + 1]; c++) {
      if (!used[c]) {
        map[c] = -1;
        continue;
      }
      if (group_mark) group_mark[count] = (int)((c - sum[r]) * nprocs + r);
      map[c] = count++;
    }
  }
  return count;
}
