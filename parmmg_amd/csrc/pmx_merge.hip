// pmx_merge.hip -- a rank's groups merged into one, on the device.
//
// pmx_merge_groups / pmx_merge_fetch / pmx_merge_maps / pmx_merge_adopt
//   <- PMMG_merge_grps (src/mergemesh_pmmg.c:967-1073): the interface points
//   (:303-469), the internal points (:480-571), the interface and internal
//   tets (:584-751) and the merged communicators (:763-935)
//
// Semantics: DESIGN.md section 4, "Group merge".  The reference is a sequence
// of passes with running counters (intvalues, tmp, flag / base); every value
// it leaves is a first occurrence or the rank of one.  With the groups'
// points, tets, node entries and face entries concatenated in group order
// (gp, gt, i, j: 0-based places in those lists):
//
//   slots    seed[slot] = the last group-0 entry naming it (atomicMax)
//   points   firstent[gp] = the first entry of point gp in its own group
//            (atomicMin): that entry is live, the others are not.  The first
//            live entry of an unseeded slot (atomicMin) creates a point; a
//            scan over the entries ranks the creators, a scan over the points
//            ranks the unlisted ones.  Every point then reads its merged id
//            from its live entry's slot, or from its rank
//   tets     tfirst[gt] = the first face entry naming tet gt (atomicMin); a
//            scan over the entries ranks the named tets in order of first
//            appearance, a scan over the tets ranks the others
//   faces    a slot holds group 0's last entry, else the first entry of a
//            later group (atomicMin) through the tet map
//   merged   the external face items in order; the external node items'
//            points by first appearance (atomicMin, a scan over the items)
//
// Orders come from indices and scans only: the atomics are min / max, whose
// result does not depend on arrival order.  No kernel waits on another
// workgroup.  Every index a kernel gathers through was range-checked by the
// host while it packed the groups -- or, for a group that a context holds, by
// pmx_merge_from.hip before it calls Merge::plan (pmx_merge.h: the plan and
// the checks and packing the two front ends share).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <vector>
#include "pmx_device.h"
#include "pmx_merge.h"

namespace {

const unsigned NONE = 0xffffffffu;

// seed[slot[i]] = the largest i < n
__global__ __launch_bounds__(256) void k_mg_last(const int *__restrict__ slot, int64_t n, int *seed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  atomicMax(&seed[slot[i]], (int)i);
}

// first[idx[i]] = the smallest i of lo <= i < hi
__global__ __launch_bounds__(256) void k_mg_first(const int *__restrict__ idx, int64_t lo, int64_t hi, unsigned *first) {
  const int64_t i = lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hi) return;
  atomicMin(&first[idx[i]], (unsigned)i);
}

struct NodeTabs {
  const int *nep, *nes, *nseed;
  const unsigned *firstent, *creator;
  int64_t n1, NN;                        // the entries of the groups >= 1: n1 <= i < NN
  __device__ __forceinline__ bool live_unseeded(int64_t i) const {
    return i >= n1 && i < NN && firstent[nep[i]] == (unsigned)i && nseed[nes[i]] < 0;
  }
};

__global__ __launch_bounds__(256) void k_mg_creator(NodeTabs t, unsigned *creator) {
  const int64_t i = t.n1 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!t.live_unseeded(i)) return;
  atomicMin(&creator[t.nes[i]], (unsigned)i);
}

struct CreatorFlag {
  NodeTabs t;
  __device__ int operator()(const int &i) const { return t.live_unseeded(i) && t.creator[t.nes[i]] == (unsigned)i; }
};
// a point of a group >= 1 that no entry of its group names
struct UnlistedFlag {
  const unsigned *first;
  int64_t lo, hi;
  __device__ int operator()(const int &k) const { return k >= lo && k < hi && first[k] == NONE; }
};
// an entry that names its element first (lo <= i < hi)
struct HeadFlag {
  const int *idx;
  const unsigned *first;
  int64_t lo, hi;
  __device__ int operator()(const int &i) const { return i >= lo && i < hi && first[idx[i]] == (unsigned)i; }
};

struct PmapArgs {
  NodeTabs t;
  const int *crank, *urank;
  int64_t P, np0, ncreate;
  int *pmap, *psrc;
};

// the merged id of every input point (meshJ->point[k].tmp) and, of the copy
// that creates a merged point, its place as that point's source
__global__ __launch_bounds__(256) void k_mg_pmap(PmapArgs a) {
  const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gp >= a.P) return;
  int m;
  bool src = true;
  if (gp < a.np0) {
    m = (int)gp + 1;
  } else if (a.t.firstent[gp] == NONE) {
    m = (int)(a.np0 + a.ncreate) + 1 + a.urank[gp];
  } else {
    const unsigned i = a.t.firstent[gp];
    const int slot = a.t.nes[i], sd = a.t.nseed[slot];
    if (sd >= 0) {
      m = a.t.nep[sd] + 1;
      src = false;
    } else {
      const unsigned c = a.t.creator[slot];
      m = (int)a.np0 + 1 + a.crank[c];
      src = c == i;
    }
  }
  a.pmap[gp] = m;
  if (src) a.psrc[m] = (int)gp;
}

// rows of the merged points: xyz (3 doubles) and the interleaved solutions
// from the creating copies; its group and local id
__global__ __launch_bounds__(256) void k_mg_points(const int *__restrict__ psrc, int64_t np, int S,
                                                   const double *__restrict__ cxyz, const double *__restrict__ csol,
                                                   double *__restrict__ mxyz, double *__restrict__ msol) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W = 3 + S;
  if (t >= np * W) return;
  const int64_t m = t / W + 1;
  const int c = (int)(t - (m - 1) * W) - 3;
  const int64_t gp = psrc[m];
  if (c < 0) mxyz[3 * m + c + 3] = cxyz[3 * gp + c + 3];
  else msol[(int64_t)S * m + c] = csol[(int64_t)S * gp + c];
}

__global__ __launch_bounds__(256) void k_mg_pinfo(const int *__restrict__ psrc, int64_t np,
                                                  const int *__restrict__ poff, int ngrp, int *__restrict__ pgrp,
                                                  int *__restrict__ pold) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (m > np) return;
  const int gp = psrc[m], g = mg_find(poff, ngrp, gp);
  pgrp[m - 1] = g;
  pold[m - 1] = gp - poff[g] + 1;
}

struct TetArgs {
  const int4 *ctet;
  const unsigned *tfirst;
  const int *hrank, *turank, *pmap, *gt;
  int64_t T;
  int ngrp;
  int *tnew, *tgrp, *told;
  int4 *mtet;
};

// tetra[k].flag of every input tet, and the merged tet it becomes
__global__ __launch_bounds__(256) void k_mg_tets(TetArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.T) return;
  const int G1 = a.ngrp + 1;
  const int *toff = a.gt + GT_T * G1, *foff = a.gt + GT_F * G1;
  const int g = mg_find(toff, a.ngrp, (int)t);
  int tn;
  if (g == 0) {
    tn = (int)t + 1;
  } else {
    const int h0 = a.hrank[foff[g]];
    const unsigned j = a.tfirst[t];
    if (j != NONE) tn = toff[g] + 1 + a.hrank[j] - h0;
    else tn = toff[g] + 1 + (a.hrank[foff[g + 1]] - h0) + a.turank[t] - a.turank[toff[g]];
  }
  const int4 v = a.ctet[t];
  a.tnew[t] = tn;
  a.mtet[tn] = make_int4(a.pmap[v.x], a.pmap[v.y], a.pmap[v.z], a.pmap[v.w]);
  a.tgrp[tn - 1] = g;
  a.told[tn - 1] = (int)t - toff[g] + 1;
}

// abs(intvalues) of the face communicator after the merge, 0: nothing filled it
__global__ __launch_bounds__(256) void k_mg_fval(const int *__restrict__ fseed, const unsigned *__restrict__ ffirst,
                                                 int64_t nitem, const int *__restrict__ fet,
                                                 const int *__restrict__ fe1, const int *__restrict__ tnew,
                                                 int *__restrict__ fval) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= nitem) return;
  const int sd = fseed[s];
  const unsigned j = ffirst[s];
  fval[s] = sd >= 0 ? fe1[sd] : j != NONE ? 12 * tnew[fet[j]] + fe1[j] % 12 : 0;
}

__global__ __launch_bounds__(256) void k_mg_extf(const int *__restrict__ extf, int64_t n, const int *__restrict__ fval,
                                                 int *__restrict__ f1, int *__restrict__ f2,
                                                 unsigned *__restrict__ ctl) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int v = fval[extf[e]];
  if (v == 0) ctl[MC_UNFILLED] = 1u;
  f1[e] = v;
  f2[e] = (int)e;
}

// the merged point of every external node item (0: an unfilled slot) and the
// first item of every such point
__global__ __launch_bounds__(256) void k_mg_extn_point(const int *__restrict__ extn, int64_t n, NodeTabs t,
                                                       const int *__restrict__ crank, int np0, int *__restrict__ em,
                                                       unsigned *pfirst, unsigned *__restrict__ ctl) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int slot = extn[e], sd = t.nseed[slot];
  const unsigned c = t.creator[slot];
  const int m = sd >= 0 ? t.nep[sd] + 1 : c != NONE ? np0 + 1 + crank[c] : 0;
  em[e] = m;
  if (m == 0) ctl[MC_UNFILLED] = 1u;
  else atomicMin(&pfirst[m], (unsigned)e);
}

struct ItemHead {
  const int *em;
  const unsigned *pfirst;
  int64_t n;
  __device__ int operator()(const int &e) const { return e < n && em[e] > 0 && pfirst[em[e]] == (unsigned)e; }
};

__global__ __launch_bounds__(256) void k_mg_extn_place(const int *__restrict__ em, int64_t n,
                                                       const unsigned *__restrict__ pfirst,
                                                       const int *__restrict__ epos, const int *__restrict__ eoff,
                                                       int next, int *__restrict__ ext_new, int *__restrict__ n1,
                                                       int *__restrict__ n2, unsigned *__restrict__ ctl) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int m = em[e];
  if (m == 0) return;
  const unsigned f = pfirst[m];
  const int pos = epos[f];
  ext_new[e] = pos;
  if (f == (unsigned)e) {
    n1[pos] = m;
    n2[pos] = pos;
  } else if (mg_find(eoff, next, (int)e) == mg_find(eoff, next, (int)f)) {
    // the communicator that gave the point its position meets it again: the
    // reference writes nothing and its item count falls short
    ctl[MC_TWICE] = 1u;
  }
}

// the interleaved solution rows 1..np into one block of np rows per solution
__global__ __launch_bounds__(256) void k_mg_deinterleave(const double *__restrict__ msol, int64_t np, SolDesc sd,
                                                         double *__restrict__ gs) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= np * sd.S) return;
  const int64_t i = t / sd.S;
  const int c = (int)(t - i * sd.S);
  int is = 0;
  while (is + 1 < sd.nsol && c >= sd.off[is + 1]) is++;
  gs[np * sd.off[is] + i * sd.size[is] + (c - sd.off[is])] = msol[(int64_t)sd.S * (i + 1) + c];
}

}  // namespace

// the packed groups are on their way to the device; the rest happens there
bool Merge::plan(int64_t nitemN, int64_t nitemF) {
  pmx_merge_plan &P = *pl;
  const int ngrp = P.ngrp, G1 = ngrp + 1, S = P.sd.S;
  const int64_t NP = P.P, T = P.T, NN = P.NN, NF = P.NF, NEN = P.NEN, NEF = P.NEF;
  const int64_t np0 = P.row(GT_P, 1), n1 = P.row(GT_N, 1), f1 = P.row(GT_F, 1);
  // slots, first occurrences
  if (!fill(P.ctl, MC_NCTL, 0, "memset") || !up(P.gtab, (const int *)P.gt.data(), (int64_t)P.gt.size(), "group table") ||
      !fill(P.nseed, nitemN, 0xff, "memset") || !fill(P.creator, nitemN, 0xff, "memset") ||
      !fill(P.fseed, nitemF, 0xff, "memset") || !fill(P.ffirst, nitemF, 0xff, "memset") ||
      !fill(P.firstent, NP, 0xff, "memset") || !fill(P.tfirst, T, 0xff, "memset"))
    return false;
  hipLaunchKernelGGL(k_mg_last, dim3(blocks(n1)), dim3(256), 0, s, (const int *)P.nes.p, n1, P.nseed.p);
  hipLaunchKernelGGL(k_mg_last, dim3(blocks(f1)), dim3(256), 0, s, (const int *)P.fe2.p, f1, P.fseed.p);
  hipLaunchKernelGGL(k_mg_first, dim3(blocks(NN - n1)), dim3(256), 0, s, (const int *)P.nep.p, n1, NN, P.firstent.p);
  hipLaunchKernelGGL(k_mg_first, dim3(blocks(NF - f1)), dim3(256), 0, s, (const int *)P.fet.p, f1, NF, P.tfirst.p);
  hipLaunchKernelGGL(k_mg_first, dim3(blocks(NF - f1)), dim3(256), 0, s, (const int *)P.fe2.p, f1, NF, P.ffirst.p);
  const NodeTabs nt{P.nep.p, P.nes.p, P.nseed.p, P.firstent.p, P.creator.p, n1, NN};
  hipLaunchKernelGGL(k_mg_creator, dim3(blocks(NN - n1)), dim3(256), 0, s, nt, P.creator.p);
  // points
  if (!scan(CreatorFlag{nt}, P.crank, NN, "creator scan") ||
      !scan(UnlistedFlag{P.firstent.p, np0, NP}, P.urank, NP, "point scan"))
    return false;
  int ncreate = 0, nunl = 0;
  if (!word(&ncreate, P.crank.p + NN, "point counts") || !word(&nunl, P.urank.p + NP, "point counts")) return false;
  P.np = np0 + ncreate + nunl;
  if (ncreate < 0 || nunl < 0 || P.np > NP) return fail("point count out of range");
  if (P.np >= (1LL << 31) - 1) return fail("merged np >= 2^31 - 1");
  const int64_t np = P.np;
  if (!pmx_dgrow(ctx, P.pmap, (size_t)NP) || !pmx_dgrow(ctx, P.psrc, (size_t)np + 1) ||
      !pmx_dgrow(ctx, P.pgrp, (size_t)np) || !pmx_dgrow(ctx, P.pold, (size_t)np) ||
      !fill(P.mxyz, 3 * (np + 1), 0, "memset") || !fill(P.msol, (np + 1) * std::max(S, 1), 0, "memset"))
    return false;
  {
    const PmapArgs a{nt, P.crank.p, P.urank.p, NP, np0, ncreate, P.pmap.p, P.psrc.p};
    hipLaunchKernelGGL(k_mg_pmap, dim3(blocks(NP)), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(k_mg_points, dim3(blocks(np * (3 + S))), dim3(256), 0, s, (const int *)P.psrc.p, np, S,
                     (const double *)P.cxyz.p, (const double *)P.csol.p, P.mxyz.p, P.msol.p);
  hipLaunchKernelGGL(k_mg_pinfo, dim3(blocks(np)), dim3(256), 0, s, (const int *)P.psrc.p, np,
                     (const int *)(P.gtab.p + GT_P * G1), ngrp, P.pgrp.p, P.pold.p);
  // tets
  if (!scan(HeadFlag{P.fet.p, P.tfirst.p, f1, NF}, P.hrank, NF, "face scan") ||
      !scan(UnlistedFlag{P.tfirst.p, (int64_t)P.row(GT_T, 1), T}, P.turank, T, "tet scan"))
    return false;
  if (!pmx_dgrow(ctx, P.tnew, (size_t)T) || !pmx_dgrow(ctx, P.tgrp, (size_t)T) || !pmx_dgrow(ctx, P.told, (size_t)T) ||
      !pmx_dgrow(ctx, P.mtet, (size_t)T + 1) || !ok(hipMemsetAsync(P.mtet.p, 0, sizeof(int4), s), "memset"))
    return false;
  {
    const TetArgs a{P.ctet.p, P.tfirst.p, P.hrank.p, P.turank.p, P.pmap.p, P.gtab.p, T, ngrp,
                    P.tnew.p, P.tgrp.p, P.told.p, P.mtet.p};
    hipLaunchKernelGGL(k_mg_tets, dim3(blocks(T)), dim3(256), 0, s, a);
  }
  // face slots, merged communicators
  if (!pmx_dgrow(ctx, P.fval, (size_t)std::max<int64_t>(nitemF, 1)) ||
      !pmx_dgrow(ctx, P.of1, (size_t)std::max<int64_t>(NEF, 1)) || !pmx_dgrow(ctx, P.of2, (size_t)std::max<int64_t>(NEF, 1)) ||
      !pmx_dgrow(ctx, P.em, (size_t)std::max<int64_t>(NEN, 1)) ||
      !pmx_dgrow(ctx, P.extn_new, (size_t)std::max<int64_t>(NEN, 1)) ||
      !pmx_dgrow(ctx, P.on1, (size_t)std::max<int64_t>(NEN, 1)) || !pmx_dgrow(ctx, P.on2, (size_t)std::max<int64_t>(NEN, 1)) ||
      !fill(P.pfirst, np + 1, 0xff, "memset"))
    return false;
  hipLaunchKernelGGL(k_mg_fval, dim3(blocks(nitemF)), dim3(256), 0, s, (const int *)P.fseed.p,
                     (const unsigned *)P.ffirst.p, nitemF, (const int *)P.fet.p, (const int *)P.fe1.p,
                     (const int *)P.tnew.p, P.fval.p);
  hipLaunchKernelGGL(k_mg_extf, dim3(blocks(NEF)), dim3(256), 0, s, (const int *)P.extf.p, NEF, (const int *)P.fval.p,
                     P.of1.p, P.of2.p, P.ctl.p);
  hipLaunchKernelGGL(k_mg_extn_point, dim3(blocks(NEN)), dim3(256), 0, s, (const int *)P.extn.p, NEN, nt,
                     (const int *)P.crank.p, (int)np0, P.em.p, P.pfirst.p, P.ctl.p);
  if (!scan(ItemHead{P.em.p, P.pfirst.p, NEN}, P.epos, NEN, "item scan")) return false;
  hipLaunchKernelGGL(k_mg_extn_place, dim3(blocks(NEN)), dim3(256), 0, s, (const int *)P.em.p, NEN,
                     (const unsigned *)P.pfirst.p, (const int *)P.epos.p, (const int *)P.eoff.p, P.next_node,
                     P.extn_new.p, P.on1.p, P.on2.p, P.ctl.p);
  unsigned h[MC_NCTL];
  int nnode = 0;
  if (!read_words(h, (const unsigned *)P.ctl.p, MC_NCTL) || !word(&nnode, P.epos.p + NEN, "node count")) return false;
  if (!ok(hipGetLastError(), "launch")) return false;
  if (h[MC_UNFILLED]) return fail("an external item names a slot that no group filled");
  if (h[MC_TWICE]) return fail("a merged point appears twice in the external node communicator of its first appearance");
  P.nnode = nnode;
  P.ne = T;
  return true;
}

// a refused or failed plan leaves none behind
int pmx_merge_refuse(pmx_ctx *ctx) {
  pmx_merge_free(ctx);
  return 0;
}

bool Merge::check_comm(int32_t ngrp, const void *groups, int nsol, const pmx_merge_comm *comm) {
  if (ngrp < 1) return fail("ngrp < 1");
  if (!groups) return fail("groups is NULL");
  if (nsol < 0 || nsol > PMX_MAX_SOLS) return fail("nsol outside 0..PMX_MAX_SOLS");
  const int64_t nitemN = comm ? comm->int_node_nitem : 0, nitemF = comm ? comm->int_face_nitem : 0;
  const int next_n = comm ? comm->next_node : 0, next_f = comm ? comm->next_face : 0;
  if (nitemN < 0 || nitemF < 0 || nitemN >= (1LL << 31) - 1 || nitemF >= (1LL << 31) - 1 || next_n < 0 || next_f < 0)
    return fail("communicator sizes out of range");
  if ((next_n > 0 && !comm->node_off) || (next_f > 0 && !comm->face_off)) return fail("a NULL view: external offsets");
  return true;
}

bool Merge::check_host_group(const pmx_merge_group &G, int g, int nsol, bool first, SolDesc &sd) {
  const std::string gs = " (group " + std::to_string(g) + ")";
  if (G.np < 1 || G.ne < 1 || G.nnode < 0 || G.nface < 0) return fail("np, ne < 1 or a negative entry count" + gs);
  if (!G.point_c || !G.tetra_v || G.point_stride < 24 || G.tetra_stride < 16 || (nsol > 0 && !G.sols) ||
      (G.nnode > 0 && (!G.node_index1 || !G.node_index2)) || (G.nface > 0 && (!G.face_index1 || !G.face_index2)))
    return fail("a NULL view or a stride too small" + gs);
  int S = 0;
  for (int i = 0; i < nsol; i++) {
    const int sz = G.sols[i].size;
    if (!G.sols[i].m) return fail("a NULL view: solution" + gs);
    if (sz != 1 && sz != 3 && sz != 6) return fail("solution size must be 1, 3 or 6" + gs);
    if (!first && sz != sd.size[i]) return fail("solution sizes differ between groups" + gs);
    sd.size[i] = sz;
    sd.off[i] = S;
    S += sz;
  }
  sd.S = S;
  return true;
}

bool Merge::check_ext(const pmx_merge_comm *comm, int64_t *pNEN, int64_t *pNEF) {
  const int next_n = comm ? comm->next_node : 0, next_f = comm ? comm->next_face : 0;
  const int64_t NEN = next_n > 0 ? comm->node_off[next_n] : 0, NEF = next_f > 0 ? comm->face_off[next_f] : 0;
  if (NEN < 0 || NEF < 0 || NEN >= (1LL << 31) - 1 || NEF >= (1LL << 31) - 1 || (NEN > 0 && !comm->node_items) ||
      (NEF > 0 && !comm->face_items))
    return fail("external items: a NULL view or counts out of range");
  for (int k = 0; k < next_n; k++)
    if (comm->node_off[k] < 0 || comm->node_off[k] > comm->node_off[k + 1] || comm->node_off[0] != 0)
      return fail("external node offsets not ascending from 0");
  for (int k = 0; k < next_f; k++)
    if (comm->face_off[k] < 0 || comm->face_off[k] > comm->face_off[k + 1] || comm->face_off[0] != 0)
      return fail("external face offsets not ascending from 0");
  *pNEN = NEN;
  *pNEF = NEF;
  return true;
}

bool Merge::pack_host_group(const pmx_merge_group &G, int g, int nsol, const SolDesc &sd, int64_t nitemN,
                            int64_t nitemF, const MergeHostDst &d) {
  const int S = sd.S;
  const int64_t p0 = d.p0, t0 = d.t0;
  const std::string gs = " (group " + std::to_string(g) + ")";
  const char *pc = (const char *)G.point_c, *tc = (const char *)G.tetra_v;
  int bad = 0;                           // 1 deleted tet, 2 vertex
  pmx_par_for(1, G.np + 1, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; i++) {
      const double *c = (const double *)(pc + i * G.point_stride);
      double *x = d.x + 3 * (i - 1);
      x[0] = c[0]; x[1] = c[1]; x[2] = c[2];
      double *r = d.s + (int64_t)S * (i - 1);
      for (int is = 0; is < nsol; is++) {
        const int sz = sd.size[is];
        const double *m = G.sols[is].m + i * sz;
        for (int j = 0; j < sz; j++) r[sd.off[is] + j] = m[j];
      }
    }
  });
  pmx_par_for(1, G.ne + 1, [&](int64_t k0, int64_t k1) {
    int b = 0;
    for (int64_t k = k0; k < k1; k++) {
      const int *v = (const int *)(tc + k * G.tetra_stride);
      if (v[0] <= 0) { b |= 1; continue; }
      int w[4];
      for (int l = 0; l < 4; l++) {
        if (v[l] < 1 || v[l] > G.np) { b |= 2; w[l] = (int)p0; }
        else w[l] = (int)(p0 + v[l] - 1);
      }
      d.t[k - 1] = make_int4(w[0], w[1], w[2], w[3]);
    }
    if (b) __atomic_fetch_or(&bad, b, __ATOMIC_RELAXED);
  });
  if (bad & 1) return fail("a deleted tet (v[0] <= 0): the reference wants packed groups" + gs);
  if (bad & 2) return fail("a vertex outside 1..np" + gs);
  return pack_entries(G, g, G.np, G.ne, p0, t0, nitemN, nitemF, d);
}

bool Merge::pack_entries(const pmx_merge_group &G, int g, int64_t np, int64_t ne, int64_t p0, int64_t t0,
                         int64_t nitemN, int64_t nitemF, const MergeHostDst &d) {
  const std::string gs = " (group " + std::to_string(g) + ")";
  int bad = 0;
  pmx_par_for(0, G.nnode, [&](int64_t i0, int64_t i1) {
    int b = 0;
    for (int64_t i = i0; i < i1; i++) {
      const int ip = G.node_index1[i], pos = G.node_index2[i];
      if (ip < 1 || ip > np) { b |= 4; continue; }
      if (pos < 0 || pos >= nitemN) { b |= 8; continue; }
      d.np[i] = (int)(p0 + ip - 1);
      d.ns[i] = pos;
    }
    if (b) __atomic_fetch_or(&bad, b, __ATOMIC_RELAXED);
  });
  pmx_par_for(0, G.nface, [&](int64_t j0, int64_t j1) {
    int b = 0;
    for (int64_t j = j0; j < j1; j++) {
      const int v = G.face_index1[j], pos = G.face_index2[j];
      if (v < 12 || (int64_t)v > 12 * ne + 11) { b |= 16; continue; }
      if (pos < 0 || pos >= nitemF) { b |= 32; continue; }
      d.ft[j] = (int)(t0 + v / 12 - 1);
      d.f1[j] = v;
      d.f2[j] = pos;
    }
    if (b) __atomic_fetch_or(&bad, b, __ATOMIC_RELAXED);
  });
  if (bad & 4) return fail("a node entry's point outside 1..np" + gs);
  if (bad & 8) return fail("a node entry's position outside 0..int_node_nitem-1" + gs);
  if (bad & 16) return fail("a face entry outside 12..12*ne+11" + gs);
  if (bad & 32) return fail("a face entry's position outside 0..int_face_nitem-1" + gs);
  return true;
}

bool Merge::pack_ext(const pmx_merge_comm *comm, int64_t nitemN, int64_t nitemF, int64_t NEN, int64_t NEF, int *hen,
                     int *hef, int *heo) {
  for (int64_t e = 0; e < NEN; e++) {
    if (comm->node_items[e] < 0 || comm->node_items[e] >= nitemN) return fail("an external node item out of range");
    hen[e] = comm->node_items[e];
  }
  for (int64_t e = 0; e < NEF; e++) {
    if (comm->face_items[e] < 0 || comm->face_items[e] >= nitemF) return fail("an external face item out of range");
    hef[e] = comm->face_items[e];
  }
  const int next_n = comm ? comm->next_node : 0;
  heo[0] = 0;
  for (int k = 0; k < next_n; k++) heo[k + 1] = (int)comm->node_off[k + 1];
  return true;
}

void pmx_merge_free(pmx_ctx *ctx) {
  pmx_merge_plan *P = ctx->merge;      // its members release themselves
  ctx->merge = nullptr;
  ctx->merge_plan_ms = ctx->merge_fetch_ms = ctx->merge_adopt_ms = -1.0;
  delete P;
}

bool pmx_merge_tet_group(pmx_ctx *ctx, const int **tgrp, int64_t *ne) {
  const pmx_merge_plan *P = ctx->merge;
  if (!P || !P->tgrp.p) return false;
  *tgrp = P->tgrp.p;
  *ne = P->ne;
  return true;
}

double pmx_merge_kernel_ms(pmx_ctx *ctx, int which) {
  return which == 16 ? ctx->merge_plan_ms : which == 17 ? ctx->merge_fetch_ms : ctx->merge_adopt_ms;
}

extern "C" {

int pmx_merge_groups(pmx_ctx *ctx, int32_t ngrp, const pmx_merge_group *groups, int nsol, const pmx_merge_comm *comm,
                     pmx_merge_sizes *sizes) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  if (ctx->merge) {
    hipStreamSynchronize(ctx->stream);
    pmx_merge_free(ctx);
  }
  ctx->merge = new pmx_merge_plan();
  Merge M{ctx, "pmx_merge_groups"};
  pmx_merge_plan &P = *ctx->merge;
  auto refuse = [&]() { return pmx_merge_refuse(ctx); };
  auto no = [&](const std::string &what) { M.fail(what); return refuse(); };
  if (!M.check_comm(ngrp, groups, nsol, comm)) return refuse();
  const int64_t nitemN = comm ? comm->int_node_nitem : 0, nitemF = comm ? comm->int_face_nitem : 0;
  const int next_n = comm ? comm->next_node : 0;
  // sizes and views
  const int G1 = ngrp + 1;
  std::vector<int64_t> off((size_t)GT_ROWS * G1, 0);
  SolDesc sd{};
  sd.nsol = nsol;
  sd.imet = -1;
  for (int g = 0; g < ngrp; g++) {
    const pmx_merge_group &G = groups[g];
    if (!M.check_host_group(G, g, nsol, g == 0, sd)) return refuse();
    off[GT_P * G1 + g + 1] = off[GT_P * G1 + g] + G.np;
    off[GT_T * G1 + g + 1] = off[GT_T * G1 + g] + G.ne;
    off[GT_N * G1 + g + 1] = off[GT_N * G1 + g] + G.nnode;
    off[GT_F * G1 + g + 1] = off[GT_F * G1 + g] + G.nface;
    if (off[GT_P * G1 + g + 1] >= (1LL << 31) - 1) return no("the groups' points together >= 2^31 - 1");
    if (12 * off[GT_T * G1 + g + 1] + 11 >= (1LL << 31)) return no("12 ne + 11 >= 2^31");
    if (off[GT_N * G1 + g + 1] >= (1LL << 31) - 1 || off[GT_F * G1 + g + 1] >= (1LL << 31) - 1)
      return no("communicator entries together >= 2^31 - 1");
  }
  const int64_t NP = off[GT_P * G1 + ngrp], T = off[GT_T * G1 + ngrp], NN = off[GT_N * G1 + ngrp],
                NF = off[GT_F * G1 + ngrp];
  int64_t NEN = 0, NEF = 0;
  if (!M.check_ext(comm, &NEN, &NEF)) return refuse();
  P.ngrp = ngrp;
  P.next_node = next_n;
  P.sd = sd;
  P.P = NP; P.T = T; P.NN = NN; P.NF = NF; P.NEN = NEN; P.NEF = NEF;
  P.gt.resize(off.size());
  for (size_t i = 0; i < off.size(); i++) P.gt[i] = (int)off[i];
  const int S = sd.S;
  // pinned staging: xyz | solutions | tets | node entries (point, slot) | face
  // entries (tet, index1, slot) | external items | external node offsets
  const size_t o_x = 0, o_s = o_x + pmx_call::al256((size_t)NP * 24),
               o_t = o_s + pmx_call::al256((size_t)NP * std::max(S, 1) * 8), o_n = o_t + pmx_call::al256((size_t)T * 16),
               o_f = o_n + pmx_call::al256((size_t)NN * 8), o_e = o_f + pmx_call::al256((size_t)NF * 12),
               o_o = o_e + pmx_call::al256((size_t)(NEN + NEF) * 4), total = o_o + pmx_call::al256((size_t)(next_n + 1) * 4);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return no("sync");   // the arena may still feed an earlier copy
  char *stg = pmx_hstage(ctx, total);
  if (!stg) return refuse();
  double *hx = (double *)(stg + o_x), *hs = (double *)(stg + o_s);
  int4 *ht = (int4 *)(stg + o_t);
  int *hnp = (int *)(stg + o_n), *hns = hnp + NN;
  int *hft = (int *)(stg + o_f), *hf1 = hft + NF, *hf2 = hf1 + NF;
  int *hen = (int *)(stg + o_e), *hef = hen + NEN, *heo = (int *)(stg + o_o);
  for (int g = 0; g < ngrp; g++) {
    const int64_t p0 = off[GT_P * G1 + g], t0 = off[GT_T * G1 + g], n0 = off[GT_N * G1 + g], f0 = off[GT_F * G1 + g];
    const MergeHostDst d{hx + 3 * p0, hs + (int64_t)S * p0, ht + t0, hnp + n0, hns + n0, hft + f0, hf1 + f0, hf2 + f0, p0, t0};
    if (!M.pack_host_group(groups[g], g, nsol, sd, nitemN, nitemF, d)) return refuse();
  }
  if (!M.pack_ext(comm, nitemN, nitemF, NEN, NEF, hen, hef, heo)) return refuse();
  // uploads, then the device
  if (!pmx_create_events(P.ev) || !M.ok(hipEventRecord(P.ev[0], M.s), "event record")) return refuse();
  if (!M.up(P.cxyz, (const double *)hx, 3 * NP, "points") || !M.up(P.csol, (const double *)hs, (int64_t)S * NP, "solutions") ||
      !M.up(P.ctet, (const int4 *)ht, T, "tets") || !M.up(P.nep, (const int *)hnp, NN, "node entries") ||
      !M.up(P.nes, (const int *)hns, NN, "node entries") || !M.up(P.fet, (const int *)hft, NF, "face entries") ||
      !M.up(P.fe1, (const int *)hf1, NF, "face entries") || !M.up(P.fe2, (const int *)hf2, NF, "face entries") ||
      !M.up(P.extn, (const int *)hen, NEN, "external items") || !M.up(P.extf, (const int *)hef, NEF, "external items") ||
      !M.up(P.eoff, (const int *)heo, next_n + 1, "external offsets"))
    return refuse();
  if (!M.plan(nitemN, nitemF)) return refuse();
  if (!M.ok(hipEventRecord(P.ev[1], M.s), "event record") || !M.sync("plan")) return refuse();
  float ms = 0.f;
  if (!M.ok(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "event time")) return refuse();
  // the inputs' device copies are not needed again
  P.cxyz.release();
  P.csol.release();
  P.ctet.release();
  ctx->merge_plan_ms = ms;
  if (sizes) {
    sizes->np = P.np;
    sizes->ne = P.ne;
    sizes->nnode = P.nnode;
    sizes->nface = NEF;
  }
  return 1;
}

int pmx_merge_fetch(pmx_ctx *ctx, const pmx_merge_out *out) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Merge M{ctx, "pmx_merge_fetch"};
  if (!ctx->merge) { M.fail("no plan: call pmx_merge_groups"); return 0; }
  if (!out) { M.fail("out is NULL"); return 0; }
  pmx_merge_plan &P = *ctx->merge;
  const SolDesc &sd = P.sd;
  const bool want_sol = out->nsol > 0;
  if (want_sol) {
    if (!out->sols || out->nsol != sd.nsol) { M.fail("nsol differs from the plan's solutions"); return 0; }
    for (int i = 0; i < sd.nsol; i++)
      if (out->sols[i].size != sd.size[i] || !out->sols[i].m) { M.fail("a solution view of another size"); return 0; }
  }
  hipStream_t s = M.s;
  const int64_t np = P.np, ne = P.ne;
  if (!M.ok(hipEventRecord(P.ev[0], s), "event record")) return 0;
  auto down = [&](void *dst, const void *d, size_t bytes) {
    if (!dst || bytes == 0) return true;
    return M.ok(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, s), "download");
  };
  if (!down(out->tetra_v ? out->tetra_v + 4 : nullptr, P.mtet.p + 1, 16 * (size_t)ne) ||
      !down(out->tet_group, P.tgrp.p, 4 * (size_t)ne) || !down(out->tet_old, P.told.p, 4 * (size_t)ne) ||
      !down(out->point_group, P.pgrp.p, 4 * (size_t)np) || !down(out->point_old, P.pold.p, 4 * (size_t)np) ||
      !down(out->xyz ? out->xyz + 3 : nullptr, P.mxyz.p + 3, 24 * (size_t)np) ||
      !down(out->node_index1, P.on1.p, 4 * (size_t)P.nnode) || !down(out->node_index2, P.on2.p, 4 * (size_t)P.nnode) ||
      !down(out->face_index1, P.of1.p, 4 * (size_t)P.NEF) || !down(out->face_index2, P.of2.p, 4 * (size_t)P.NEF) ||
      !down(out->ext_node_items, P.extn_new.p, 4 * (size_t)P.NEN) || !down(out->ext_face_items, P.of2.p, 4 * (size_t)P.NEF))
    return 0;
  if (want_sol && sd.S > 0) {
    if (!pmx_dgrow(ctx, P.gs, (size_t)(sd.S * np))) return 0;
    hipLaunchKernelGGL(k_mg_deinterleave, dim3(Merge::blocks(np * sd.S)), dim3(256), 0, s, (const double *)P.msol.p, np,
                       sd, P.gs.p);
    for (int i = 0; i < sd.nsol; i++)
      if (!down(out->sols[i].m + sd.size[i], P.gs.p + np * sd.off[i], 8 * (size_t)(np * sd.size[i]))) return 0;
  }
  if (!M.ok(hipEventRecord(P.ev[1], s), "event record") || !M.sync("fetch")) return 0;
  float ms = 0.f;
  if (!M.ok(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "event time")) return 0;
  ctx->merge_fetch_ms = ms;
  return 1;
}

int pmx_merge_maps(pmx_ctx *ctx, int32_t g, int *point_new, int *tet_new) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Merge M{ctx, "pmx_merge_maps"};
  if (!ctx->merge) { M.fail("no plan: call pmx_merge_groups"); return 0; }
  pmx_merge_plan &P = *ctx->merge;
  if (g < 0 || g >= P.ngrp) { M.fail("group out of range"); return 0; }
  // a plan of pmx_merge_groups_from: the maps in the sources' own numbering
  const bool own = !P.uoff.empty();
  const int64_t p0 = own ? P.uoff[g] : P.row(GT_P, g), p1 = own ? P.uoff[g + 1] : P.row(GT_P, g + 1);
  const int64_t t0 = own ? P.uoff[P.ngrp + 1 + g] : P.row(GT_T, g), t1 = own ? P.uoff[P.ngrp + 2 + g] : P.row(GT_T, g + 1);
  const int *pm = own ? P.upmap.p : P.pmap.p, *tm = own ? P.utnew.p : P.tnew.p;
  if (point_new && !M.ok(hipMemcpyAsync(point_new, pm + p0, 4 * (size_t)(p1 - p0), hipMemcpyDeviceToHost, M.s), "download"))
    return 0;
  if (tet_new && !M.ok(hipMemcpyAsync(tet_new, tm + t0, 4 * (size_t)(t1 - t0), hipMemcpyDeviceToHost, M.s), "download"))
    return 0;
  return M.sync("maps") ? 1 : 0;
}

int pmx_merge_adopt(pmx_ctx *ctx, int imet) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Merge M{ctx, "pmx_merge_adopt"};
  if (!ctx->merge) { M.fail("no plan: call pmx_merge_groups"); return 0; }
  pmx_merge_plan &P = *ctx->merge;
  if (imet < -1 || imet >= P.sd.nsol) { M.fail("imet outside -1..nsol-1"); return 0; }
  ctx->merge_adopt_ms = -1.0;
  if (!M.ok(hipEventRecord(P.ev[0], M.s), "event record")) return 0;
  SolDesc sd = P.sd;
  sd.imet = imet;
  // rows as they are (no gather), no surface: a merged group needs none
  const AdoptSrc src{P.mtet.p + 1, P.mxyz.p, P.msol.p, nullptr, false, 0.0};
  if (!pmx_ctx_adopt_group(ctx, "pmx_merge_adopt", src, sd, P.np, P.ne)) return 0;
  if (!M.ok(hipEventRecord(P.ev[1], M.s), "event record") || !M.sync("adopt")) return 0;
  float ms = 0.f;
  if (!M.ok(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "event time")) return 0;
  ctx->merge_adopt_ms = ms;
  return 1;
}

int pmx_merge_release(pmx_ctx *ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  pmx_merge_free(ctx);
  return 1;
}

}  // extern "C"
