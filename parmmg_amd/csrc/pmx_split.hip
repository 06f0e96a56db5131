// pmx_split.hip -- the uploaded group split by a partition, on the device.
//
// pmx_split_groups / pmx_split_fetch <- PMMG_split_eachGrp
//   (src/grpsplit_pmmg.c:1267-1445): PMMG_splitGrps_countTetPerGrp
//   (:1106-1116), PMMG_splitGrps_fillGroup (:819-1094) and the communicator
//   updates it calls (:606-795)
// pmx_split_adopt <- PMMG_update_oldGrps (src/libparmmg1.c:653) for one new
//   group: it becomes another context's background, on the device
//
// Semantics: DESIGN.md section 4, "Group split".  The reference is one
// sequential pass with running counters; here every order and counter is a
// rank or a prefix count (p: a tet's place in the stable order by part, the
// groups' tets one after the other; q = 4 p + slot):
//
//   tets     stable radix sort of the tet numbers by part -> tcat[p], the
//            groups' offsets toff[g] by binary search, tet_new by a scatter
//   points   first[v] = min q over the tets holding v (atomicMin): the first
//            visit of v in the first group that holds it.  An occurrence of v
//            in another group goes to a side list (a select in q order), sorted
//            stably by (group, vertex): the head of a run is that group's first
//            visit.  First visits flagged over q, an exclusive scan ranks them:
//            rank[q] is the point's place in the concatenated point arrays
//   remap    one thread per p: local vertex ids, the adjacency through
//            tet_new, the cut-face flags, and per point of a cut face the
//            smallest 12 j + 3 f + poi (the second loop's first encounter) and
//            per vertex the smallest group in which it lies on a cut face
//   faces    entries flagged over (p, f); the owner of a cut face is its side
//            in the smaller group; two exclusive scans give the place in the
//            group's list and the position in the internal communicator
//   nodes    per point its class (listed by the first loop / appended by the
//            second / not listed), a scan over the first class, a select and a
//            sort by (group, first encounter) of the second
//
// Orders come from keys and scans only: the atomics are min / max, whose
// result does not depend on arrival order.  No kernel waits on another
// workgroup.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "pmx_device.h"
#include "pmx_internal.h"

typedef unsigned long long u64;

namespace {

// control words
enum { SC_PART = 0, SC_DELETED = 1, SC_BADREC = 2, SC_FACE = 3, SC_LOOKUP = 4, SC_NSEL = 5, SC_NCTL = 8 };
// rows of the group table (ngrp + 1 entries each): tets, points, face
// entries, owned cut faces, first-loop node entries, second-loop node entries
// of the groups before g
enum { GT_T = 0, GT_P = 1, GT_F = 2, GT_O = 3, GT_A = 4, GT_C = 5, GT_ROWS = 6 };

__constant__ int SP_IDIR[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};

__device__ __forceinline__ int comp4(const int4 &v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

struct U8Bit {
  int sh;
  __host__ __device__ int operator()(const uint8_t &x) const { return (x >> sh) & 1; }
};

// part values, deleted tets, records that point outside the mesh; iota[k-1] = k
__global__ __launch_bounds__(256) void k_sp_check(const TetRec *__restrict__ tets, int64_t ne, int64_t np,
                                                  const int *__restrict__ part, int ngrp, int *__restrict__ iota,
                                                  unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne) return;
  iota[k - 1] = (int)k;
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  const int4 v = recs[2 * k], nb = recs[2 * k + 1];
  const int g = part[k];
  if (g < 0 || g >= ngrp) ctl[SC_PART] = 1u;
  if (v.x <= 0) ctl[SC_DELETED] = 1u;
  const int n = (int)ne, m = (int)np;
  if (nb.x < 0 || nb.x > n || nb.y < 0 || nb.y > n || nb.z < 0 || nb.z > n || nb.w < 0 || nb.w > n || v.x > m ||
      v.y < 1 || v.y > m || v.z < 1 || v.z > m || v.w < 1 || v.w > m)
    ctl[SC_BADREC] = 1u;
}

// gt[GT_T][g] = the first place of part g in the sorted keys, g = 0..ngrp
__global__ __launch_bounds__(256) void k_sp_toff(const unsigned *__restrict__ gcat, int64_t ne, int ngrp,
                                                 int *__restrict__ gt) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g > ngrp) return;
  int64_t lo = 0, hi = ne;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (gcat[mid] < (unsigned)g) lo = mid + 1;
    else hi = mid;
  }
  gt[g] = (int)lo;
}

__global__ __launch_bounds__(256) void k_sp_tnew(const int *__restrict__ tcat, const unsigned *__restrict__ gcat,
                                                 const int *__restrict__ toff, int64_t ne, int *__restrict__ tnew) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= ne) return;
  tnew[tcat[p]] = (int)p - toff[gcat[p]] + 1;
}

__global__ __launch_bounds__(256) void k_sp_first(const TetRec *__restrict__ tets, const int *__restrict__ tcat,
                                                  int64_t ne, unsigned *first) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= ne) return;
  const int4 v = reinterpret_cast<const int4 *>(tets)[2 * (int64_t)tcat[p]];
  const unsigned q = 4u * (unsigned)p;
  atomicMin(&first[v.x], q);
  atomicMin(&first[v.y], q + 1);
  atomicMin(&first[v.z], q + 2);
  atomicMin(&first[v.w], q + 3);
}

// q is an occurrence of its vertex in a group other than the vertex's first
struct SideSel {
  const int4 *recs;
  const int *tcat;
  const unsigned *gcat, *first;
  __device__ bool operator()(const unsigned &q) const {
    const unsigned p = q >> 2;
    const int4 v = recs[2 * (int64_t)tcat[p]];
    return gcat[first[comp4(v, q & 3)] >> 2] != gcat[p];
  }
};

__global__ __launch_bounds__(256) void k_sp_sidekey(const unsigned *__restrict__ side, int64_t n,
                                                    const TetRec *__restrict__ tets, const int *__restrict__ tcat,
                                                    const unsigned *__restrict__ gcat, u64 *__restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned q = side[i], p = q >> 2;
  const int4 v = reinterpret_cast<const int4 *>(tets)[2 * (int64_t)tcat[p]];
  key[i] = ((u64)gcat[p] << 32) | (unsigned)comp4(v, q & 3);
}

__global__ __launch_bounds__(256) void k_sp_flag_first(const unsigned *__restrict__ first, int64_t np,
                                                       uint8_t *__restrict__ ff) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (v > np) return;
  const unsigned q = first[v];
  if (q != 0xffffffffu) ff[q] = 1;
}

__global__ __launch_bounds__(256) void k_sp_flag_side(const u64 *__restrict__ key, const unsigned *__restrict__ val,
                                                      int64_t n, uint8_t *__restrict__ ff) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (i == 0 || key[i - 1] != key[i]) ff[val[i]] = 1;
}

// dst[g] = pos[mul * src[g]], g = 0..ngrp
__global__ __launch_bounds__(256) void k_sp_gtab(const int *__restrict__ pos, const int *__restrict__ src, int mul,
                                                 int ngrp, int *__restrict__ dst) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g > ngrp) return;
  dst[g] = pos[(int64_t)mul * src[g]];
}

__global__ __launch_bounds__(256) void k_sp_pcat(const uint8_t *__restrict__ ff, const int *__restrict__ rank,
                                                 const TetRec *__restrict__ tets, const int *__restrict__ tcat,
                                                 const unsigned *__restrict__ gcat, int64_t nq,
                                                 int *__restrict__ pcat, int *__restrict__ pgrp) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq || !ff[q]) return;
  const int64_t p = q >> 2;
  const int4 v = reinterpret_cast<const int4 *>(tets)[2 * (int64_t)tcat[p]];
  const int r = rank[q];
  pcat[r] = comp4(v, (int)(q & 3));
  pgrp[r] = (int)gcat[p];
}

struct Lookup {
  const unsigned *first, *gcat;
  const int *rank;
  const u64 *skey;
  const unsigned *sval;
  int64_t nside;
  // the place of (g, v) in the concatenated point arrays, -1 when (g, v) is no point
  __device__ __forceinline__ int operator()(unsigned g, int v) const {
    const unsigned fq = first[v];
    if (gcat[fq >> 2] == g) return rank[fq];
    const u64 key = ((u64)g << 32) | (unsigned)v;
    int64_t lo = 0, hi = nside;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (skey[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= nside || skey[lo] != key) return -1;
    return rank[sval[lo]];
  }
};

struct RemapArgs {
  const TetRec *tets;
  const int *tcat;
  const unsigned *gcat;
  const int *part, *tnew, *toff, *poff, *fold;
  int64_t ne;
  Lookup look;
  int4 *vcat, *acat;
  uint8_t *fl;
  unsigned *ckey;
  int *mincut;
  unsigned *ctl;
};

// the face of tet nb that looks at tet k
__device__ __forceinline__ int sp_back_face(const int4 *recs, int nb, int k) {
  const int4 n = recs[2 * (int64_t)nb + 1];
  return n.x == k ? 0 : n.y == k ? 1 : n.z == k ? 2 : n.w == k ? 3 : -1;
}

__global__ __launch_bounds__(256) void k_sp_remap(RemapArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.ne) return;
  const int4 *recs = reinterpret_cast<const int4 *>(a.tets);
  const int k = a.tcat[p];
  const unsigned g = a.gcat[p];
  const int j = (int)p - a.toff[g] + 1, pg = a.poff[g];
  const int4 v4 = recs[2 * (int64_t)k], nb4 = recs[2 * (int64_t)k + 1];
  const int vv[4] = {v4.x, v4.y, v4.z, v4.w}, nbs[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
  int P[4];
  bool bad = false;
#pragma unroll
  for (int s = 0; s < 4; s++) {
    P[s] = a.look(g, vv[s]);
    if (P[s] < 0) { bad = true; P[s] = pg; }
  }
  a.vcat[p] = make_int4(P[0] - pg + 1, P[1] - pg + 1, P[2] - pg + 1, P[3] - pg + 1);
  int ad[4];
  unsigned flw = 0;
#pragma unroll
  for (int f = 0; f < 4; f++) {
    const int nb = nbs[f];
    ad[f] = 0;
    if (nb == 0) {
      if (a.fold && a.fold[4 * (int64_t)k + f] >= 0) flw |= 1u << (8 * f);
      continue;
    }
    const int gn = a.part[nb];
    if ((unsigned)gn == g) {
      const int fb = sp_back_face(recs, nb, k);
      if (fb < 0) bad = true;
      ad[f] = 4 * a.tnew[nb] + (fb < 0 ? 0 : fb);
    } else {
      flw |= (1u | (g < (unsigned)gn ? 2u : 0u)) << (8 * f);
      for (int poi = 0; poi < 3; poi++) {
        const int s = SP_IDIR[f][poi];
        atomicMin(&a.ckey[P[s]], (unsigned)(12 * j + 3 * f + poi));
        atomicMin(&a.mincut[vv[s]], (int)g);
      }
    }
  }
  a.acat[p] = make_int4(ad[0], ad[1], ad[2], ad[3]);
  reinterpret_cast<unsigned *>(a.fl)[p] = flw;
  if (bad) a.ctl[SC_LOOKUP] = 1u;
}

struct FaceArgs {
  const TetRec *tets;
  const int *tcat;
  const unsigned *gcat;
  const int *part, *tnew, *toff, *fold, *in1, *in2;
  int64_t ne;
  const uint8_t *fl;
  const int *epos, *opos;
  int nitem0;
  int *f1, *f2;
};

__global__ __launch_bounds__(256) void k_sp_faces(FaceArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.ne) return;
  const unsigned flw = reinterpret_cast<const unsigned *>(a.fl)[p];
  if (!(flw & 0x01010101u)) return;
  const int4 *recs = reinterpret_cast<const int4 *>(a.tets);
  const int k = a.tcat[p];
  const unsigned g = a.gcat[p];
  const int j = (int)p - a.toff[g] + 1;
  const int4 v4 = recs[2 * (int64_t)k], nb4 = recs[2 * (int64_t)k + 1];
  const int vv[4] = {v4.x, v4.y, v4.z, v4.w}, nbs[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
  for (int f = 0; f < 4; f++) {
    const unsigned fl = (flw >> (8 * f)) & 0xffu;
    if (!(fl & 1u)) continue;
    const int e = a.epos[4 * p + f];
    const int nb = nbs[f];
    int iploc, pos;
    if (nb == 0) {                         // a face of the old communicator
      const int i = a.fold[4 * (int64_t)k + f];
      iploc = (a.in1[i] % 12) % 3;
      pos = a.in2[i];
    } else if (fl & 2u) {                  // first side: it imposes the starting point
      iploc = 0;
      pos = a.nitem0 + a.opos[4 * p + f];
    } else {
      const int gn = a.part[nb];
      const int64_t pn = (int64_t)a.toff[gn] + a.tnew[nb] - 1;
      int fb = sp_back_face(recs, nb, k);
      if (fb < 0) fb = 0;
      pos = a.nitem0 + a.opos[4 * pn + fb];
      const int ip = comp4(recs[2 * (int64_t)nb], SP_IDIR[fb][0]);
      iploc = vv[SP_IDIR[f][0]] == ip ? 0 : vv[SP_IDIR[f][1]] == ip ? 1 : 2;
    }
    a.f1[e] = 12 * j + 3 * f + iploc;
    a.f2[e] = pos;
  }
}

// input communicators: the last entry of a face / node wins, as in the
// reference's loops; a listed face with a neighbour raises SC_FACE
__global__ __launch_bounds__(256) void k_sp_fold(const int *__restrict__ in1, int64_t n,
                                                 const TetRec *__restrict__ tets, int *fold,
                                                 unsigned *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ie = in1[i] / 12, fac = (in1[i] % 12) / 3;
  if (comp4(reinterpret_cast<const int4 *>(tets)[2 * (int64_t)ie + 1], fac) != 0) ctl[SC_FACE] = 1u;
  atomicMax(&fold[4 * (int64_t)ie + fac], (int)i);
}

__global__ __launch_bounds__(256) void k_sp_inidx(const int *__restrict__ in1, int64_t n, int *inidx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  atomicMax(&inidx[in1[i]], (int)i);
}

// bit 0: listed by the first loop (the vertex carries a value when the group
// copies it); bit 1: appended by the second loop
__global__ __launch_bounds__(256) void k_sp_nodeflag(const int *__restrict__ pcat, const int *__restrict__ pgrp,
                                                     int64_t NP, const int *__restrict__ inidx,
                                                     const int *__restrict__ mincut,
                                                     const unsigned *__restrict__ ckey, uint8_t *__restrict__ af) {
  const int64_t P = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (P >= NP) return;
  const int v = pcat[P];
  const bool A = (inidx && inidx[v] >= 0) || mincut[v] < pgrp[P];
  af[P] = A ? 1 : (ckey[P] != 0xffffffffu ? 2 : 0);
}

__global__ __launch_bounds__(256) void k_sp_ckey(const int *__restrict__ clist, int64_t n,
                                                 const int *__restrict__ pgrp, const unsigned *__restrict__ ckey,
                                                 u64 *__restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int P = clist[i];
  key[i] = ((u64)(unsigned)pgrp[P] << 32) | ckey[P];
}

// gt[GT_A][g] = first-loop entries before group g, gt[GT_C][g] = second-loop ones
__global__ __launch_bounds__(256) void k_sp_ntab(const int *__restrict__ apos, const u64 *__restrict__ ckey64,
                                                 int64_t nC, int ngrp, int *__restrict__ gt) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g > ngrp) return;
  gt[GT_A * (ngrp + 1) + g] = apos[gt[GT_P * (ngrp + 1) + g]];
  const u64 key = (u64)(unsigned)g << 32;
  int64_t lo = 0, hi = nC;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ckey64[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  gt[GT_C * (ngrp + 1) + g] = (int)lo;
}

// the second loop's i-th append over all groups: nitem stands at nitem0 + (all
// entries of the groups before g) + (g's first-loop entries) + (its rank in g)
// = nitem0 + aoff[g + 1] + i
__global__ __launch_bounds__(256) void k_sp_node_c(const u64 *__restrict__ key, const int *__restrict__ cval,
                                                   int64_t nC, const int *__restrict__ pcat,
                                                   const int *__restrict__ gt, int ngrp, int nitem0,
                                                   int *__restrict__ newval, int *__restrict__ n1,
                                                   int *__restrict__ n2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nC) return;
  const int g = (int)(key[i] >> 32), P = cval[i];
  const int val = nitem0 + gt[GT_A * (ngrp + 1) + g + 1] + (int)i + 1;
  newval[pcat[P]] = val;
  const int64_t at = (int64_t)gt[GT_A * (ngrp + 1) + g + 1] + i;
  n1[at] = P - gt[GT_P * (ngrp + 1) + g] + 1;
  n2[at] = val;
}

__global__ __launch_bounds__(256) void k_sp_node_a(const uint8_t *__restrict__ af, const int *__restrict__ apos,
                                                   const int *__restrict__ pcat, const int *__restrict__ pgrp,
                                                   int64_t NP, const int *__restrict__ inidx,
                                                   const int *__restrict__ in2, const int *__restrict__ newval,
                                                   const int *__restrict__ gt, int ngrp, int *__restrict__ n1,
                                                   int *__restrict__ n2) {
  const int64_t P = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (P >= NP || !(af[P] & 1)) return;
  const int v = pcat[P], g = pgrp[P];
  const int i = inidx ? inidx[v] : -1;
  const int64_t at = (int64_t)gt[GT_C * (ngrp + 1) + g] + apos[P];
  n1[at] = (int)P - gt[GT_P * (ngrp + 1) + g] + 1;
  n2[at] = i >= 0 ? in2[i] : newval[v];
}

// the xyz rows (3 doubles) of the points idx[0..n) into gx, and their rows of
// the interleaved solutions into gs, one block of n rows per solution
// (solution i at n * off[i]): each block is one copy into the caller's array
__global__ __launch_bounds__(256) void k_sp_gather(const int *__restrict__ idx, int64_t n,
                                                   const double *__restrict__ xyz, const double *__restrict__ sol,
                                                   SolDesc sd, double *__restrict__ gx, double *__restrict__ gs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W = 3 + sd.S;
  if (t >= n * W) return;
  const int64_t i = t / W;
  const int c = (int)(t - i * W) - 3;
  const int64_t v = idx[i];
  if (c < 0) {
    gx[3 * i + c + 3] = xyz[3 * v + c + 3];
    return;
  }
  int is = 0;
  while (is + 1 < sd.nsol && c >= sd.off[is + 1]) is++;
  gs[n * sd.off[is] + i * sd.size[is] + (c - sd.off[is])] = sol[(int64_t)sd.S * v + c];
}

}  // namespace

struct pmx_split_plan {
  int64_t ne = 0, np = 0, NP = 0, NF = 0, NN = 0;
  int ngrp = 0;
  std::vector<int> gt;                   // the group table, GT_ROWS x (ngrp + 1)
  DevBuf<int> part, iota, tcat, tnew, rank, pcat, pgrp, epos, opos, apos, f1, f2, n1, n2, gtab, fold, inidx,
      newval, mincut, clist, cval, in_f1, in_f2, in_n1, in_n2;
  DevBuf<int4> vcat, acat;
  DevBuf<unsigned> gcat, first, ckey, side, sval, ctl;
  DevBuf<u64> skey, skey2, ckey64, ckey64b;
  DevBuf<uint8_t> ff, fl, af;
  DevBuf<char> tmp;
  DevBuf<double> gx, gs;
  DevEvent ev[2];
  int row(int r, int g) const { return gt[(size_t)r * (ngrp + 1) + g]; }
};

namespace {

struct Split : pmx_call {
  pmx_split_plan *pl;
  Split(pmx_ctx *c, const char *w) : pmx_call{c, w, c->stream}, pl(c->split) {}

  // the stream synchronised and checked for launch errors
  bool read_ctl(unsigned *h) {
    return ok(hipMemcpyAsync(h, pl->ctl.p, sizeof(unsigned) * SC_NCTL, hipMemcpyDeviceToHost, s), "control words") &&
           sync("control words");
  }
  bool up(DevBuf<int> &d, const int *h, int64_t n, const char *what) {
    return pmx_dgrow(ctx, d, (size_t)std::max<int64_t>(n, 1)) &&
           (n == 0 || ok(hipMemcpyAsync(d.p, h, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s), what));
  }
  bool gtab_down() {
    return ok(hipMemcpyAsync(pl->gt.data(), pl->gtab.p, sizeof(int) * pl->gt.size(), hipMemcpyDeviceToHost, s),
              "group table") &&
           sync("group table");
  }

  // part: the host's array (ne ints), uploaded into the plan's buffer; NULL:
  // dpart, a partition on the device (ne + 1 ints, tet k at k), read where it
  // lies -- the plan only reads the partition, and only while it is built
  bool plan(const int32_t *part, const int *dpart, int ngrp, const pmx_split_comm *comm);
};

static int bits_for(u64 maxval) {
  int b = 1;
  while (b < 64 && (maxval >> b)) b++;
  return b;
}

bool Split::plan(const int32_t *part, const int *dpart, int ngrp, const pmx_split_comm *comm) {
  pmx_split_plan &P = *pl;
  const int64_t ne = ctx->ne, np = ctx->np, nq = 4 * ne;
  const TetRec *tets = ctx->d_tets.p;
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  const int64_t nface = comm ? comm->nface : 0, nnode = comm ? comm->nnode : 0;
  const int64_t fn0 = comm ? comm->int_face_nitem : 0, nn0 = comm ? comm->int_node_nitem : 0;
  const int G1 = ngrp + 1;
  unsigned h[SC_NCTL];
  P.ne = ne;
  P.np = np;
  P.ngrp = ngrp;
  P.gt.assign((size_t)GT_ROWS * G1, 0);
  const size_t n1 = (size_t)(ne + 1);
  if ((part && !pmx_dgrow(ctx, P.part, n1)) || !pmx_dgrow(ctx, P.iota, n1) || !pmx_dgrow(ctx, P.tcat, n1) ||
      !pmx_dgrow(ctx, P.tnew, n1) || !pmx_dgrow(ctx, P.gcat, n1) || !pmx_dgrow(ctx, P.ctl, SC_NCTL) ||
      !pmx_dgrow(ctx, P.gtab, (size_t)GT_ROWS * G1) || !pmx_dgrow(ctx, P.first, (size_t)(np + 1)) ||
      !pmx_dgrow(ctx, P.mincut, (size_t)(np + 1)) || !pmx_dgrow(ctx, P.newval, (size_t)(np + 1)) ||
      !pmx_dgrow(ctx, P.side, (size_t)nq) || !pmx_dgrow(ctx, P.ff, (size_t)nq + 4) ||
      !pmx_dgrow(ctx, P.fl, (size_t)nq + 4) || !pmx_dgrow(ctx, P.rank, (size_t)nq + 1) ||
      !pmx_dgrow(ctx, P.epos, (size_t)nq + 1) || !pmx_dgrow(ctx, P.opos, (size_t)nq + 1) ||
      !pmx_dgrow(ctx, P.vcat, n1) || !pmx_dgrow(ctx, P.acat, n1))
    return false;
  if (!pmx_create_events(P.ev)) return fail("event");
  if (!ok(hipEventRecord(P.ev[0], s), "event record")) return false;
  if (!ok(hipMemsetAsync(P.ctl.p, 0, sizeof(unsigned) * SC_NCTL, s), "memset") ||
      !ok(hipMemsetAsync(P.gtab.p, 0, sizeof(int) * (size_t)GT_ROWS * G1, s), "memset") ||
      (part && !ok(hipMemcpyAsync(P.part.p + 1, part, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, s), "part upload")))
    return false;
  if (part) dpart = P.part.p;
  hipLaunchKernelGGL(k_sp_check, dim3(blocks(ne)), dim3(256), 0, s, tets, ne, np, dpart, ngrp,
                     P.iota.p, P.ctl.p);
  if (!read_ctl(h)) return false;
  if (h[SC_DELETED]) return fail("a deleted tet (v[0] <= 0): the reference wants a packed mesh");
  if (h[SC_BADREC]) return fail("a tet record with a neighbour outside 0..ne or a vertex outside 1..np");
  if (h[SC_PART]) return fail("a part value outside 0..ngrp-1");

  // input communicators
  const bool have_f = nface > 0, have_n = nnode > 0;
  if (have_f) {
    if (!up(P.in_f1, comm->face_index1, nface, "face upload") || !up(P.in_f2, comm->face_index2, nface, "face upload") ||
        !pmx_dgrow(ctx, P.fold, 4 * n1) || !ok(hipMemsetAsync(P.fold.p, 0xff, sizeof(int) * 4 * n1, s), "memset"))
      return false;
    hipLaunchKernelGGL(k_sp_fold, dim3(blocks(nface)), dim3(256), 0, s, (const int *)P.in_f1.p, nface, tets,
                       P.fold.p, P.ctl.p);
  }
  if (have_n) {
    if (!up(P.in_n1, comm->node_index1, nnode, "node upload") || !up(P.in_n2, comm->node_index2, nnode, "node upload") ||
        !pmx_dgrow(ctx, P.inidx, (size_t)(np + 1)) ||
        !ok(hipMemsetAsync(P.inidx.p, 0xff, sizeof(int) * (size_t)(np + 1), s), "memset"))
      return false;
    hipLaunchKernelGGL(k_sp_inidx, dim3(blocks(nnode)), dim3(256), 0, s, (const int *)P.in_n1.p, nnode, P.inidx.p);
  }

  // tets: the stable order by part
  if (!sort_pairs(P.tmp, (const unsigned *)(dpart + 1), P.gcat.p, (const int *)P.iota.p, P.tcat.p, ne,
                  bits_for((u64)ngrp), "tet sort"))
    return false;
  int *gt = P.gtab.p;
  hipLaunchKernelGGL(k_sp_toff, dim3(blocks(G1)), dim3(256), 0, s, (const unsigned *)P.gcat.p, ne, ngrp, gt);
  hipLaunchKernelGGL(k_sp_tnew, dim3(blocks(ne)), dim3(256), 0, s, (const int *)P.tcat.p, (const unsigned *)P.gcat.p,
                     (const int *)gt, ne, P.tnew.p);
  if (!read_ctl(h)) return false;
  if (h[SC_FACE]) return fail("an input face entry on a face whose adjacency is not 0");
  if (!gtab_down()) return false;
  for (int g = 0; g < ngrp; g++) {
    const int64_t neg = (int64_t)P.row(GT_T, g + 1) - P.row(GT_T, g);
    if (neg <= 0) return fail("part " + std::to_string(g) + " is empty");
    if (12 * neg + 11 >= (1LL << 31)) return fail("12 ne_g + 11 >= 2^31 in part " + std::to_string(g));
  }

  // points: first visits
  if (!ok(hipMemsetAsync(P.first.p, 0xff, sizeof(unsigned) * (size_t)(np + 1), s), "memset") ||
      !ok(hipMemsetAsync(P.ff.p, 0, (size_t)nq + 4, s), "memset") ||
      !ok(hipMemsetAsync(P.fl.p, 0, (size_t)nq + 4, s), "memset"))
    return false;
  hipLaunchKernelGGL(k_sp_first, dim3(blocks(ne)), dim3(256), 0, s, tets, (const int *)P.tcat.p, ne, P.first.p);
  {
    hipcub::CountingInputIterator<unsigned> it(0u);
    const SideSel sel{recs, P.tcat.p, P.gcat.p, P.first.p};
    if (!select_if(P.tmp, it, P.side.p, P.ctl.p + SC_NSEL, nq, sel, "side select")) return false;
  }
  if (!read_ctl(h)) return false;
  const int64_t nside = h[SC_NSEL];
  if (nside > nq) return fail("side list out of range");
  if (!pmx_dgrow(ctx, P.skey, (size_t)nside + 1) || !pmx_dgrow(ctx, P.skey2, (size_t)nside + 1) ||
      !pmx_dgrow(ctx, P.sval, (size_t)nside + 1))
    return false;
  if (nside > 0) {
    hipLaunchKernelGGL(k_sp_sidekey, dim3(blocks(nside)), dim3(256), 0, s, (const unsigned *)P.side.p, nside, tets,
                       (const int *)P.tcat.p, (const unsigned *)P.gcat.p, P.skey.p);
    if (!sort_pairs(P.tmp, (const u64 *)P.skey.p, P.skey2.p, (const unsigned *)P.side.p, P.sval.p, nside,
                    32 + bits_for((u64)ngrp), "side sort"))
      return false;
    hipLaunchKernelGGL(k_sp_flag_side, dim3(blocks(nside)), dim3(256), 0, s, (const u64 *)P.skey2.p,
                       (const unsigned *)P.sval.p, nside, P.ff.p);
  }
  hipLaunchKernelGGL(k_sp_flag_first, dim3(blocks(np)), dim3(256), 0, s, (const unsigned *)P.first.p, np, P.ff.p);
  {
    hipcub::TransformInputIterator<int, U8Bit, const uint8_t *> in((const uint8_t *)P.ff.p, U8Bit{0});
    if (!exclusive_sum(P.tmp, in, P.rank.p, nq + 1, "point scan")) return false;
  }
  hipLaunchKernelGGL(k_sp_gtab, dim3(blocks(G1)), dim3(256), 0, s, (const int *)P.rank.p, (const int *)gt, 4, ngrp,
                     gt + GT_P * G1);
  if (!gtab_down()) return false;
  P.NP = P.row(GT_P, ngrp);
  if (P.NP < 1 || P.NP > nq) return fail("point count out of range");
  const size_t NP1 = (size_t)P.NP + 1;
  if (!pmx_dgrow(ctx, P.pcat, NP1) || !pmx_dgrow(ctx, P.pgrp, NP1) || !pmx_dgrow(ctx, P.ckey, NP1) ||
      !pmx_dgrow(ctx, P.af, NP1 + 3) || !pmx_dgrow(ctx, P.apos, NP1) || !pmx_dgrow(ctx, P.clist, NP1) ||
      !pmx_dgrow(ctx, P.cval, NP1) || !pmx_dgrow(ctx, P.ckey64, NP1) || !pmx_dgrow(ctx, P.ckey64b, NP1) ||
      !pmx_dgrow(ctx, P.n1, NP1) || !pmx_dgrow(ctx, P.n2, NP1))
    return false;
  hipLaunchKernelGGL(k_sp_pcat, dim3(blocks(nq)), dim3(256), 0, s, (const uint8_t *)P.ff.p, (const int *)P.rank.p,
                     tets, (const int *)P.tcat.p, (const unsigned *)P.gcat.p, nq, P.pcat.p, P.pgrp.p);

  // remap
  if (!ok(hipMemsetAsync(P.ckey.p, 0xff, sizeof(unsigned) * NP1, s), "memset") ||
      !ok(hipMemsetAsync(P.af.p, 0, NP1 + 3, s), "memset"))
    return false;
  {
    // mincut: 0x7f7f7f7f, above every group number
    if (!ok(hipMemsetAsync(P.mincut.p, 0x7f, sizeof(int) * (size_t)(np + 1), s), "memset")) return false;
    RemapArgs a{tets, P.tcat.p, P.gcat.p, dpart, P.tnew.p, gt, gt + GT_P * G1, have_f ? P.fold.p : nullptr, ne,
                Lookup{P.first.p, P.gcat.p, P.rank.p, P.skey2.p, P.sval.p, nside},
                P.vcat.p, P.acat.p, P.fl.p, P.ckey.p, P.mincut.p, P.ctl.p};
    hipLaunchKernelGGL(k_sp_remap, dim3(blocks(ne)), dim3(256), 0, s, a);
  }

  // faces
  {
    hipcub::TransformInputIterator<int, U8Bit, const uint8_t *> e((const uint8_t *)P.fl.p, U8Bit{0});
    hipcub::TransformInputIterator<int, U8Bit, const uint8_t *> o((const uint8_t *)P.fl.p, U8Bit{1});
    if (!exclusive_sum(P.tmp, e, P.epos.p, nq + 1, "face scan") || !exclusive_sum(P.tmp, o, P.opos.p, nq + 1, "owner scan")) return false;
  }
  hipLaunchKernelGGL(k_sp_gtab, dim3(blocks(G1)), dim3(256), 0, s, (const int *)P.epos.p, (const int *)gt, 4, ngrp,
                     gt + GT_F * G1);
  hipLaunchKernelGGL(k_sp_gtab, dim3(blocks(G1)), dim3(256), 0, s, (const int *)P.opos.p, (const int *)gt, 4, ngrp,
                     gt + GT_O * G1);

  // nodes
  hipLaunchKernelGGL(k_sp_nodeflag, dim3(blocks(P.NP)), dim3(256), 0, s, (const int *)P.pcat.p,
                     (const int *)P.pgrp.p, P.NP, have_n ? (const int *)P.inidx.p : nullptr, (const int *)P.mincut.p,
                     (const unsigned *)P.ckey.p, P.af.p);
  {
    hipcub::TransformInputIterator<int, U8Bit, const uint8_t *> in((const uint8_t *)P.af.p, U8Bit{0});
    if (!exclusive_sum(P.tmp, in, P.apos.p, P.NP + 1, "node scan")) return false;
    hipcub::CountingInputIterator<int> it(0);
    hipcub::TransformInputIterator<int, U8Bit, const uint8_t *> fl((const uint8_t *)P.af.p, U8Bit{1});
    if (!select_flagged(P.tmp, it, fl, P.clist.p, P.ctl.p + SC_NSEL, P.NP, "node select")) return false;
  }
  if (!read_ctl(h)) return false;
  if (h[SC_LOOKUP]) return fail("inconsistent tet records (a vertex without a number, or a one-sided adjacency)");
  const int64_t nC = h[SC_NSEL];
  if (nC > P.NP) return fail("node list out of range");
  if (nC > 0) {
    hipLaunchKernelGGL(k_sp_ckey, dim3(blocks(nC)), dim3(256), 0, s, (const int *)P.clist.p, nC,
                       (const int *)P.pgrp.p, (const unsigned *)P.ckey.p, P.ckey64.p);
    if (!sort_pairs(P.tmp, (const u64 *)P.ckey64.p, P.ckey64b.p, (const int *)P.clist.p, P.cval.p, nC,
                    32 + bits_for((u64)ngrp), "node sort"))
      return false;
  }
  hipLaunchKernelGGL(k_sp_ntab, dim3(blocks(G1)), dim3(256), 0, s, (const int *)P.apos.p, (const u64 *)P.ckey64b.p,
                     nC, ngrp, gt);
  if (!gtab_down()) return false;
  P.NF = P.row(GT_F, ngrp);
  P.NN = (int64_t)P.row(GT_A, ngrp) + nC;
  if (P.NF < 0 || P.NF > nq || P.NN > P.NP) return fail("list sizes out of range");
  if (fn0 + P.row(GT_O, ngrp) >= (1LL << 31) || nn0 + P.NN + 1 >= (1LL << 31))
    return fail("a communicator position >= 2^31");
  if (!pmx_dgrow(ctx, P.f1, (size_t)P.NF + 1) || !pmx_dgrow(ctx, P.f2, (size_t)P.NF + 1)) return false;
  {
    FaceArgs a{tets, P.tcat.p, P.gcat.p, dpart, P.tnew.p, gt, have_f ? P.fold.p : nullptr,
               have_f ? P.in_f1.p : nullptr, have_f ? P.in_f2.p : nullptr, ne, P.fl.p, P.epos.p, P.opos.p, (int)fn0,
               P.f1.p, P.f2.p};
    hipLaunchKernelGGL(k_sp_faces, dim3(blocks(ne)), dim3(256), 0, s, a);
  }
  if (nC > 0)
    hipLaunchKernelGGL(k_sp_node_c, dim3(blocks(nC)), dim3(256), 0, s, (const u64 *)P.ckey64b.p,
                       (const int *)P.cval.p, nC, (const int *)P.pcat.p, (const int *)gt, ngrp, (int)nn0,
                       P.newval.p, P.n1.p, P.n2.p);
  hipLaunchKernelGGL(k_sp_node_a, dim3(blocks(P.NP)), dim3(256), 0, s, (const uint8_t *)P.af.p,
                     (const int *)P.apos.p, (const int *)P.pcat.p, (const int *)P.pgrp.p, P.NP,
                     have_n ? (const int *)P.inidx.p : nullptr, have_n ? (const int *)P.in_n2.p : nullptr,
                     (const int *)P.newval.p, (const int *)gt, ngrp, P.n1.p, P.n2.p);
  if (!ok(hipEventRecord(P.ev[1], s), "event record") || !sync("plan")) return false;
  float ms = 0.f;
  if (!ok(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "event time")) return false;
  ctx->split_plan_ms = ms;
  return true;
}

}  // namespace

void pmx_split_free(pmx_ctx *ctx) {
  pmx_split_plan *P = ctx->split;      // its members release themselves
  ctx->split = nullptr;
  ctx->split_valid = false;
  ctx->split_plan_ms = ctx->split_fetch_ms = -1.0;
  delete P;
}

double pmx_split_kernel_ms(pmx_ctx *ctx, int which) {
  return which == 14 ? ctx->split_plan_ms : which == 15 ? ctx->split_fetch_ms : ctx->split_adopt_ms;
}

// pmx_split_groups and pmx_split_groups_part: part, the host's array, or --
// device -- the context's partition (ngrp is then the partition's)
static int split_groups(pmx_ctx *ctx, const char *who, const int32_t *part, bool device, int32_t ngrp,
                        const pmx_split_comm *comm, pmx_split_sizes *sizes, int *tet_new, int64_t *int_face_nitem,
                        int64_t *int_node_nitem) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  ctx->split_valid = false;
  ctx->split_plan_ms = ctx->split_fetch_ms = -1.0;
  if (!ctx->split) ctx->split = new pmx_split_plan();
  Split S{ctx, who};
  if (!ctx->have_bg) { S.fail("upload a group first"); return 0; }
  const int64_t ne = ctx->ne, np = ctx->np;
  if (4 * ne >= (1LL << 31)) { S.fail("4 ne >= 2^31 (32-bit indices)"); return 0; }
  const int *dpart = nullptr;
  if (device) {
    if (!pmx_part_held(ctx, &dpart, &ngrp)) {
      S.fail("no partition: call pmx_part_from_marks or pmx_part_upload");
      return 0;
    }
  } else if (!part) { S.fail("part is NULL"); return 0; }
  if (ngrp < 1) { S.fail("ngrp < 1"); return 0; }
  if ((int64_t)ngrp > ne) { S.fail("more parts than tets: a part is empty"); return 0; }
  if (comm) {
    if (comm->nface < 0 || comm->nnode < 0 || comm->int_face_nitem < 0 || comm->int_node_nitem < 0 ||
        (comm->nface > 0 && (!comm->face_index1 || !comm->face_index2)) ||
        (comm->nnode > 0 && (!comm->node_index1 || !comm->node_index2))) {
      S.fail("communicator counts < 0 or arrays missing");
      return 0;
    }
    for (int64_t i = 0; i < comm->nface; i++)
      if (comm->face_index1[i] < 12 || (int64_t)comm->face_index1[i] > 12 * ne + 11) {
        S.fail("an input face entry outside 12..12*ne+11");
        return 0;
      }
    for (int64_t i = 0; i < comm->nnode; i++)
      if (comm->node_index1[i] < 1 || comm->node_index1[i] > np) {
        S.fail("an input node outside 1..np");
        return 0;
      }
  }
  if (!S.plan(part, dpart, ngrp, comm)) return 0;
  const pmx_split_plan &P = *ctx->split;
  std::vector<int> tn;
  if (tet_new) {
    tn.resize((size_t)ne);
    if (hipMemcpyAsync(tn.data(), P.tnew.p + 1, sizeof(int) * (size_t)ne, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
        hipStreamSynchronize(S.s) != hipSuccess) {
      S.fail("tet_new download");
      return 0;
    }
    std::copy(tn.begin(), tn.end(), tet_new);
  }
  if (sizes)
    for (int g = 0; g < ngrp; g++) {
      sizes[g].ne = P.row(GT_T, g + 1) - P.row(GT_T, g);
      sizes[g].np = P.row(GT_P, g + 1) - P.row(GT_P, g);
      sizes[g].nface = P.row(GT_F, g + 1) - P.row(GT_F, g);
      sizes[g].nnode = (P.row(GT_A, g + 1) - P.row(GT_A, g)) + (P.row(GT_C, g + 1) - P.row(GT_C, g));
    }
  if (int_face_nitem) *int_face_nitem = (comm ? comm->int_face_nitem : 0) + P.row(GT_O, ngrp);
  if (int_node_nitem) *int_node_nitem = (comm ? comm->int_node_nitem : 0) + P.NN;
  ctx->split_valid = true;
  return 1;
}

extern "C" {

int pmx_split_groups(pmx_ctx *ctx, const int32_t *part, int32_t ngrp, const pmx_split_comm *comm,
                     pmx_split_sizes *sizes, int *tet_new, int64_t *int_face_nitem, int64_t *int_node_nitem) {
  return split_groups(ctx, "pmx_split_groups", part, false, ngrp, comm, sizes, tet_new, int_face_nitem, int_node_nitem);
}

int pmx_split_groups_part(pmx_ctx *ctx, const pmx_split_comm *comm, pmx_split_sizes *sizes, int *tet_new,
                          int64_t *int_face_nitem, int64_t *int_node_nitem) {
  return split_groups(ctx, "pmx_split_groups_part", nullptr, true, 0, comm, sizes, tet_new, int_face_nitem,
                      int_node_nitem);
}

int pmx_split_fetch(pmx_ctx *ctx, int32_t g, const pmx_split_out *out) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Split S{ctx, "pmx_split_fetch"};
  if (!ctx->split || !ctx->split_valid) {
    S.fail("no plan: call pmx_split_groups (a background upload or promotion drops the plan)");
    return 0;
  }
  pmx_split_plan &P = *ctx->split;
  if (g < 0 || g >= P.ngrp) { S.fail("group out of range"); return 0; }
  if (!out) { S.fail("out is NULL"); return 0; }
  const int64_t t0 = P.row(GT_T, g), neg = P.row(GT_T, g + 1) - t0;
  const int64_t p0 = P.row(GT_P, g), npg = P.row(GT_P, g + 1) - p0;
  const int64_t f0 = P.row(GT_F, g), nf = P.row(GT_F, g + 1) - f0;
  const int64_t n0 = (int64_t)P.row(GT_A, g) + P.row(GT_C, g);
  const int64_t nn = (int64_t)P.row(GT_A, g + 1) + P.row(GT_C, g + 1) - n0;
  const SolDesc &sd = ctx->sd;
  const bool want_sol = out->nsol > 0;
  if (want_sol) {
    if (!out->sols || out->nsol != sd.nsol) { S.fail("nsol differs from the uploaded solutions"); return 0; }
    for (int i = 0; i < sd.nsol; i++)
      if (out->sols[i].size != sd.size[i] || !out->sols[i].m) { S.fail("a solution view of another size"); return 0; }
  }
  hipStream_t s = S.s;
  const bool want_x = out->xyz != nullptr;
  // Straight into the caller's arrays: every refusal has been decided above,
  // only a device error can stop the copies now (and may leave them partial).
  if (!S.ok(hipEventRecord(P.ev[0], s), "event record")) return 0;
  auto down = [&](int *dst, const int *d, int64_t n) {
    if (!dst || n <= 0) return true;
    return S.ok(hipMemcpyAsync(dst, d, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s), "download");
  };
  if (!down(out->tet_old, P.tcat.p + t0, neg) ||
      !down(out->tetra_v ? out->tetra_v + 4 : nullptr, reinterpret_cast<const int *>(P.vcat.p + t0), 4 * neg) ||
      !down(out->adja ? out->adja + 1 : nullptr, reinterpret_cast<const int *>(P.acat.p + t0), 4 * neg) ||
      !down(out->point_old, P.pcat.p + p0, npg) || !down(out->face_index1, P.f1.p + f0, nf) ||
      !down(out->face_index2, P.f2.p + f0, nf) || !down(out->node_index1, P.n1.p + n0, nn) ||
      !down(out->node_index2, P.n2.p + n0, nn))
    return 0;
  SolDesc gsd = sd;
  if (!want_sol) gsd.nsol = gsd.S = 0;
  if ((want_x || want_sol) && npg > 0) {
    if (!pmx_dgrow(ctx, P.gx, (size_t)(3 * npg)) || !pmx_dgrow(ctx, P.gs, (size_t)std::max<int64_t>(gsd.S * npg, 1)))
      return 0;
    hipLaunchKernelGGL(k_sp_gather, dim3(Split::blocks(npg * (3 + gsd.S))), dim3(256), 0, s,
                       (const int *)(P.pcat.p + p0), npg, (const double *)ctx->d_xyz.p, (const double *)ctx->d_sol.p,
                       gsd, P.gx.p, P.gs.p);
    if (want_x &&
        !S.ok(hipMemcpyAsync(out->xyz + 3, P.gx.p, sizeof(double) * (size_t)(3 * npg), hipMemcpyDeviceToHost, s),
              "download"))
      return 0;
    for (int i = 0; i < gsd.nsol; i++)
      if (!S.ok(hipMemcpyAsync(out->sols[i].m + gsd.size[i], P.gs.p + npg * gsd.off[i],
                               sizeof(double) * (size_t)(npg * gsd.size[i]), hipMemcpyDeviceToHost, s),
                "download"))
        return 0;
  }
  if (!S.ok(hipEventRecord(P.ev[1], s), "event record") || !S.sync("fetch")) return 0;
  float ms = 0.f;
  if (!S.ok(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "event time")) return 0;
  ctx->split_fetch_ms = ms;
  if (out->adja) {
    out->adja[0] = 0;
    for (int i = 1; i <= 4; i++) out->adja[4 * neg + i] = 0;
  }
  return 1;
}

// Group g of src's plan as dst's background: the rows through the plan's
// point_old slice, the connectivity from its vcat slice, everything else as
// any adopt (pmx_ctx_adopt_group).  dst's stream waits for src's; the call
// returns once dst's copies are done (finish_background synchronises), so src
// may release or replace its plan afterwards.
int pmx_split_adopt(pmx_ctx *src, int32_t g, pmx_ctx *dst, int imet, int surface, double hausd) {
  if (!dst) {
    pmx_set_noctx_error("pmx_split_adopt: dst is NULL");
    return 0;
  }
  const pmx_call C{dst, "pmx_split_adopt", dst->stream};
  dst->split_adopt_ms = -1.0;
  if (!src) return C.fail("src is NULL");
  if (src == dst) return C.fail("dst is src: a context cannot adopt from its own plan (the install drops it)");
  if (src->device != dst->device) return C.fail("src and dst are on different devices");
  if (!src->split || !src->split_valid || !src->have_bg)
    return C.fail("no plan on src: call pmx_split_groups (a background upload or promotion drops the plan)");
  const pmx_split_plan &P = *src->split;
  if (g < 0 || g >= P.ngrp) return C.fail("group out of range");
  if (imet < -1 || imet >= src->sd.nsol) return C.fail("imet outside -1..nsol-1");
  if (surface != 0 && surface != 1) return C.fail("surface must be 0 or 1");
  if (!std::isfinite(hausd) || hausd < 0.0) return C.fail("hausd must be finite and >= 0");
  hipSetDevice(dst->device);
  const int64_t t0 = P.row(GT_T, g), neg = P.row(GT_T, g + 1) - t0;
  const int64_t p0 = P.row(GT_P, g), npg = P.row(GT_P, g + 1) - p0;
  SolDesc sd = src->sd;
  sd.imet = imet;
  sd.metric_const = 0;
  if (!pmx_create_events(dst->adopt_ev) || !dst->ev_give.create(false)) return C.fail("event");
  // everything src's stream has queued (the plan, a fetch's gather) is done
  // before dst's stream reads src's buffers
  PMX_CK(C, hipEventRecord(dst->ev_give, src->stream));
  PMX_CK(C, hipStreamWaitEvent(dst->stream, dst->ev_give, 0));
  PMX_CK(C, hipEventRecord(dst->adopt_ev[0], dst->stream));
  const AdoptSrc from{P.vcat.p + t0, src->d_xyz.p, src->d_sol.p, P.pcat.p + p0, surface == 1, hausd};
  if (!pmx_ctx_adopt_group(dst, "pmx_split_adopt", from, sd, npg, neg)) return 0;
  PMX_CK(C, hipEventRecord(dst->adopt_ev[1], dst->stream));
  if (!C.sync("adopt")) return 0;
  float ms = 0.f;
  PMX_CK(C, hipEventElapsedTime(&ms, dst->adopt_ev[0], dst->adopt_ev[1]));
  dst->split_adopt_ms = ms;
  return 1;
}

int pmx_split_release(pmx_ctx *ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  pmx_split_free(ctx);
  return 1;
}

}  // extern "C"
