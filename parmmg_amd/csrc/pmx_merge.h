// pmx_merge.h -- the merge plan and the call helper its two front ends share
// (host code, and the kernels' bisection): pmx_merge_groups (pmx_merge.hip, every group from host views)
// and pmx_merge_groups_from (pmx_merge_from.hip, groups that contexts hold).
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <string>
#include <vector>
#include "pmx_internal.h"

// control words of Merge::plan
enum { MC_UNFILLED = 0, MC_TWICE = 1, MC_NCTL = 4 };
// rows of the group table (ngrp + 1 entries each): points, tets, node
// entries, face entries of the groups before g
enum { GT_P = 0, GT_T = 1, GT_N = 2, GT_F = 3, GT_ROWS = 4 };

// the last i with tab[i] <= x, tab ascending with tab[0] <= x (n entries)
__device__ __forceinline__ int mg_find(const int *__restrict__ tab, int n, int x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct pmx_merge_plan {
  int64_t P = 0, T = 0, NN = 0, NF = 0, NEN = 0, NEF = 0, np = 0, ne = 0, nnode = 0;
  int ngrp = 0, next_node = 0;
  SolDesc sd{};
  std::vector<int> gt;                   // the group table, GT_ROWS x (ngrp + 1)
  DevBuf<double> cxyz, csol, mxyz, msol, gs;
  DevBuf<int4> ctet, mtet;
  DevBuf<int> gtab, nep, nes, fet, fe1, fe2, extn, extf, eoff, nseed, fseed, crank, urank, hrank, turank, pmap,
      psrc, pgrp, pold, tnew, tgrp, told, fval, em, epos, extn_new, on1, on2, of1, of2;
  DevBuf<unsigned> firstent, creator, tfirst, ffirst, pfirst, ctl;
  DevBuf<char> tmp;
  DevEvent ev[2];
  // pmx_merge_groups_from: the sources in their own numbering, one after the
  // other (a held group with its unused points and deleted tets).  uoff: the
  // points, then the tets of the sources before g (ngrp + 1 entries each);
  // upmap / utnew: the maps pmx_merge_maps returns, 0 for a dropped entity.
  // Empty for a plan of pmx_merge_groups, whose groups are merged as they are
  std::vector<int64_t> uoff;
  DevBuf<int> upmap, utnew;
  int row(int r, int g) const { return gt[(size_t)r * (ngrp + 1) + g]; }
};

// where one host group's packed rows go: the pointers at the group's first
// row or entry, p0 / t0 the places those rows take among all groups' rows
struct MergeHostDst {
  double *x, *s;
  int4 *t;
  int *np, *ns, *ft, *f1, *f2;
  int64_t p0, t0;
};

struct Merge : pmx_call {
  pmx_merge_plan *pl;
  Merge(pmx_ctx *c, const char *w) : pmx_call{c, w, c->stream}, pl(c->merge) {}

  template <class T> bool up(DevBuf<T> &d, const T *h, int64_t n, const char *what) {
    return pmx_dgrow(ctx, d, (size_t)std::max<int64_t>(n, 1)) &&
           (n == 0 || ok(hipMemcpyAsync(d.p, h, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s), what));
  }
  template <class T> bool fill(DevBuf<T> &d, int64_t n, int byte, const char *what) {
    return pmx_dgrow(ctx, d, (size_t)std::max<int64_t>(n, 1)) &&
           ok(hipMemsetAsync(d.p, byte, sizeof(T) * (size_t)std::max<int64_t>(n, 1), s), what);
  }
  template <class F> bool scan(F f, DevBuf<int> &out, int64_t n, const char *what) {
    hipcub::CountingInputIterator<int> it(0);
    hipcub::TransformInputIterator<int, F, hipcub::CountingInputIterator<int>> in(it, f);
    return pmx_dgrow(ctx, out, (size_t)n + 1) && exclusive_sum(pl->tmp, in, out.p, n + 1, what);
  }
  bool word(int *dst, const int *src, const char *what) { return read_words(dst, src, 1, what); }

  // the call's arguments other than the groups; false: refused (fail() called)
  bool check_comm(int32_t ngrp, const void *groups, int nsol, const pmx_merge_comm *comm);
  // one host group's views: NULL views, strides, solution sizes (sd.size /
  // off / S filled by group `first`, compared by the others)
  bool check_host_group(const pmx_merge_group &G, int g, int nsol, bool first, SolDesc &sd);
  // the external communicators' offsets; NEN / NEF: their items
  bool check_ext(const pmx_merge_comm *comm, int64_t *NEN, int64_t *NEF);
  // a host group's rows and entries packed into the staging, range-checked
  bool pack_host_group(const pmx_merge_group &G, int g, int nsol, const SolDesc &sd, int64_t nitemN, int64_t nitemF,
                       const MergeHostDst &d);
  // its node and face entries alone, range-checked against np / ne and staged
  // as p0 + point - 1 and t0 + tet - 1 (a held group: its own sizes, p0 = t0 = 0)
  bool pack_entries(const pmx_merge_group &G, int g, int64_t np, int64_t ne, int64_t p0, int64_t t0, int64_t nitemN,
                    int64_t nitemF, const MergeHostDst &d);
  // the external items range-checked into hen / hef, the node offsets into heo
  bool pack_ext(const pmx_merge_comm *comm, int64_t nitemN, int64_t nitemF, int64_t NEN, int64_t NEF, int *hen,
                int *hef, int *heo);
  // cxyz, csol, ctet and the entry arrays are on their way to the device;
  // the rest happens there (pmx_merge.hip)
  bool plan(int64_t nitemN, int64_t nitemF);
};

// a refused or failed plan leaves none behind; returns 0
int pmx_merge_refuse(pmx_ctx *ctx);
