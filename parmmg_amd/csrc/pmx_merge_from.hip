// pmx_merge_from.hip -- a merge whose groups lie in contexts on the device.
//
// pmx_merge_groups_from
//   <- the two merges of PMMG_split_n2mGrps (src/loadbalancing_pmmg.c:88,135),
//   whose groups the device already holds: PMMG_merge_grps' skips of unused
//   points and deleted tets (src/mergemesh_pmmg.c:346,507,710) numbered as
//   PMMG_mark_packedTetra (src/libparmmg1.c:102-113, 245-248) packs a group
//
// Semantics: DESIGN.md section 4, "Merge from held groups".  With every
// source's points and tets in its own numbering, one source after the other
// (u, ut: 0-based places in those lists; a host source has every point used
// and every tet valid):
//
//   marks    used[u] = 1 where a valid tet of the held group names the point,
//            tval[ut] = 1 for a valid tet (plain stores of 1)
//   scans    prank[u], trank[ut]: the place among the used points / valid
//            tets before it -- the stable packing of every group and, the
//            groups being in order, its place in the merge's concatenated
//            lists.  The group table is the ranks at the sources' offsets
//   gather   a held group's vertex and solution rows and its remapped
//            connectivity into the plan's cxyz / csol / ctet, its entries
//            through the ranks; host sources are packed and uploaded there.
//            Marks and gathers are one launch each over all sources: a
//            thread finds its source by bisection of the offsets and reads
//            the holder's pointers from a descriptor table
//   plan     Merge::plan, unchanged (pmx_merge.hip)
//   back     tet_old / point_old and both maps through the ranks again, in
//            the sources' own numbering
//
// Orders come from indices and scans only; the atomics are min (the smallest
// group with an error).  No kernel waits on another workgroup.  Every index a
// kernel gathers through is range-checked first: a held tet's vertices by the
// mark pass (whose result the host reads before any gather is launched), the
// entries by the host against the holder's np and ne.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <string>
#include <vector>
#include "pmx_device.h"
#include "pmx_merge.h"

namespace {

const unsigned NOGRP = 0xffffffffu;
// control words: the smallest group with a vertex out of range, with a node
// entry on a dropped point, with a face entry on a dropped tet
enum { FC_BADV = 0, FC_DROPN = 1, FC_DROPF = 2, FC_NCTL = 4 };

// the connectivity half of a 32-B tet record: one 16-B load
__device__ __forceinline__ int4 mf_tet(const TetRec *__restrict__ tets, int64_t k) {
  return *reinterpret_cast<const int4 *>(&tets[k]);
}

// One source as the kernels see it: a holder's rows (row i at 3 i / S i, tets
// 1-based), or held = 0 for a host source, which the kernels skip
struct HeldDesc {
  const double *xyz, *sol;
  const TetRec *tets;
  int np, held;
};
// every source: the descriptors, the offsets of the sources' points and tets
// in their own numbering (ngrp + 1 each) and of their node and face entries
struct HeldTabs {
  const HeldDesc *desc;
  const int *uoffP, *uoffT, *eoffN, *eoffF;
  int ngrp;
  uint8_t *used, *tval;
  const int *prank, *trank;
};

// one launch over the tets of all sources: a group by bisection
__global__ __launch_bounds__(256) void k_mf_mark(HeldTabs h, int64_t UT, unsigned *ctl) {
  const int64_t ut = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (ut >= UT) return;
  const int g = mg_find(h.uoffT, h.ngrp, (int)ut);
  const HeldDesc d = h.desc[g];
  if (!d.held) return;
  const int np = d.np;
  const int4 v = mf_tet(d.tets, ut - h.uoffT[g] + 1);
  bool valid = v.x > 0;
  if (valid && (v.x > np || v.y < 1 || v.y > np || v.z < 1 || v.z > np || v.w < 1 || v.w > np)) {
    atomicMin(&ctl[FC_BADV], (unsigned)g);
    valid = false;
  }
  h.tval[ut] = valid ? 1 : 0;
  if (!valid) return;
  uint8_t *used = h.used + h.uoffP[g] - 1;
  used[v.x] = 1;
  used[v.y] = 1;
  used[v.z] = 1;
  used[v.w] = 1;
}

struct ByteFlag {
  const uint8_t *f;
  int64_t n;
  __device__ int operator()(const int &i) const { return i < n && f[i] != 0; }
};

// out[i] = rank[at[i]]: the ranks at the sources' offsets (points, then tets)
__global__ __launch_bounds__(256) void k_mf_table(const int *__restrict__ prank, const int *__restrict__ trank,
                                                  const int *__restrict__ at, int G1, int *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * G1) return;
  out[i] = i < G1 ? prank[at[i]] : trank[at[i]];
}

// rows of the used points of the held sources: one lane per row element
// (xyz, then the solutions)
__global__ __launch_bounds__(256) void k_mf_points(HeldTabs h, int64_t UP, int S, double *__restrict__ cxyz,
                                                   double *__restrict__ csol) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W = 3 + S;
  if (t >= UP * W) return;
  const int64_t u = t / W;
  if (!h.used[u]) return;
  const int g = mg_find(h.uoffP, h.ngrp, (int)u);
  const HeldDesc d = h.desc[g];
  if (!d.held) return;
  const int64_t i = u - h.uoffP[g] + 1;
  const int c = (int)(t - u * W) - 3;
  const int64_t gp = h.prank[u];
  if (c < 0) cxyz[3 * gp + c + 3] = d.xyz[3 * i + c + 3];
  else csol[(int64_t)S * gp + c] = d.sol[(int64_t)S * i + c];
}

// the valid tets, their vertices as places among all groups' packed points
__global__ __launch_bounds__(256) void k_mf_tets(HeldTabs h, int64_t UT, int4 *__restrict__ ctet) {
  const int64_t ut = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (ut >= UT || !h.tval[ut]) return;
  const int g = mg_find(h.uoffT, h.ngrp, (int)ut);
  const HeldDesc d = h.desc[g];
  if (!d.held) return;
  const int4 v = mf_tet(d.tets, ut - h.uoffT[g] + 1);
  const int *r = h.prank + h.uoffP[g] - 1;
  ctet[h.trank[ut]] = make_int4(r[v.x], r[v.y], r[v.z], r[v.w]);
}

// node entries of the held sources: the own point id - 1 becomes the point's
// place among all groups' packed points
__global__ __launch_bounds__(256) void k_mf_node_entries(HeldTabs h, int64_t NN, int *__restrict__ nep, unsigned *ctl) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= NN) return;
  const int g = mg_find(h.eoffN, h.ngrp, (int)e);
  if (!h.desc[g].held) return;
  const int64_t u0 = h.uoffP[g], u = u0 + nep[e];
  if (h.used[u]) {
    nep[e] = h.prank[u];
  } else {
    atomicMin(&ctl[FC_DROPN], (unsigned)g);
    nep[e] = h.prank[u0];
  }
}

// face entries: the tet's place among all groups' valid tets, and index1 with
// the tet's id in the packed group
__global__ __launch_bounds__(256) void k_mf_face_entries(HeldTabs h, int64_t NF, int *__restrict__ fet,
                                                         int *__restrict__ fe1, unsigned *ctl) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= NF) return;
  const int g = mg_find(h.eoffF, h.ngrp, (int)e);
  if (!h.desc[g].held) return;
  const int64_t ut0 = h.uoffT[g], ut = ut0 + fet[e];
  const int t0 = h.trank[ut0];
  if (h.tval[ut]) {
    const int gt = h.trank[ut];
    fet[e] = gt;
    fe1[e] = 12 * (gt - t0 + 1) + fe1[e] % 12;
  } else {
    atomicMin(&ctl[FC_DROPF], (unsigned)g);
    fet[e] = t0;
    fe1[e] = 12;
  }
}

struct BackArgs {
  const uint8_t *flag;
  const int *rank, *map, *grp, *uoff;    // the merged id of a packed place; the group of a merged entity
  const int *psrc;                       // points: the packed place that created a merged point; tets: nullptr
  int64_t n;
  int *umap, *old;
};

// the maps in the sources' own numbering, and the own id of every merged
// entity (of a point: of the copy that created it)
__global__ __launch_bounds__(256) void k_mf_back(BackArgs a) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= a.n) return;
  if (!a.flag[u]) {
    a.umap[u] = 0;
    return;
  }
  const int p = a.rank[u], m = a.map[p];
  a.umap[u] = m;
  if (!a.psrc || a.psrc[m] == p) a.old[m - 1] = (int)(u - a.uoff[a.grp[m - 1]]) + 1;
}

}  // namespace

extern "C" {

int pmx_merge_groups_from(pmx_ctx *ctx, int32_t ngrp, const pmx_merge_source *src, int nsol,
                          const pmx_merge_comm *comm, pmx_merge_sizes *sizes) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  if (ctx->merge) {
    hipStreamSynchronize(ctx->stream);
    pmx_merge_free(ctx);
  }
  ctx->merge = new pmx_merge_plan();
  Merge M{ctx, "pmx_merge_groups_from"};
  pmx_merge_plan &P = *ctx->merge;
  auto refuse = [&]() { return pmx_merge_refuse(ctx); };
  auto no = [&](const std::string &what) { M.fail(what); return refuse(); };
  if (!M.check_comm(ngrp, src, nsol, comm)) return refuse();
  const int64_t nitemN = comm ? comm->int_node_nitem : 0, nitemF = comm ? comm->int_face_nitem : 0;
  const int next_n = comm ? comm->next_node : 0;
  // sizes and views: the sources in their own numbering (uoff), the entries
  const int G1 = ngrp + 1;
  std::vector<int64_t> uoff((size_t)2 * G1, 0), eoff((size_t)2 * G1, 0);
  SolDesc sd{};
  sd.nsol = nsol;
  sd.imet = -1;
  int64_t HP = 0, HT = 0;                // the host sources' points and tets
  bool any_held = false;
  for (int g = 0; g < ngrp; g++) {
    const pmx_merge_group &G = src[g].g;
    const pmx_ctx *H = src[g].held;
    const std::string gs = " (group " + std::to_string(g) + ")";
    int64_t npg, neg;
    if (!H) {
      if (!M.check_host_group(G, g, nsol, g == 0, sd)) return refuse();
      npg = G.np;
      neg = G.ne;
      HP += npg;
      HT += neg;
    } else {
      if (!H->have_bg) return no("the holder has no background" + gs);
      if (H->device != ctx->device) return no("the holder is on another device" + gs);
      if (H->sd.nsol != nsol) return no("the holder's nsol differs from the call's" + gs);
      if (G.nnode < 0 || G.nface < 0) return no("np, ne < 1 or a negative entry count" + gs);
      if ((G.nnode > 0 && (!G.node_index1 || !G.node_index2)) || (G.nface > 0 && (!G.face_index1 || !G.face_index2)))
        return no("a NULL view or a stride too small" + gs);
      int S = 0;
      for (int i = 0; i < nsol; i++) {
        const int sz = H->sd.size[i];
        if (g > 0 && sz != sd.size[i]) return no("the holder's solution sizes differ from the call's" + gs);
        sd.size[i] = sz;
        sd.off[i] = S;
        S += sz;
      }
      sd.S = S;
      npg = H->np;
      neg = H->ne;
      if (npg < 1 || neg < 1) return no("np, ne < 1 or a negative entry count" + gs);
      any_held = true;
    }
    uoff[g + 1] = uoff[g] + npg;
    uoff[G1 + g + 1] = uoff[G1 + g] + neg;
    eoff[g + 1] = eoff[g] + G.nnode;
    eoff[G1 + g + 1] = eoff[G1 + g] + G.nface;
    if (uoff[g + 1] >= (1LL << 31) - 1) return no("the groups' points together >= 2^31 - 1");
    if (12 * uoff[G1 + g + 1] + 11 >= (1LL << 31)) return no("12 ne + 11 >= 2^31");
    if (eoff[g + 1] >= (1LL << 31) - 1 || eoff[G1 + g + 1] >= (1LL << 31) - 1)
      return no("communicator entries together >= 2^31 - 1");
  }
  const int64_t UP = uoff[ngrp], UT = uoff[G1 + ngrp], NN = eoff[ngrp], NF = eoff[G1 + ngrp];
  int64_t NEN = 0, NEF = 0;
  if (!M.check_ext(comm, &NEN, &NEF)) return refuse();
  const int S = sd.S;
  // pinned staging: the host sources' xyz | solutions | tets, then as in
  // pmx_merge_groups the entries, the external items and offsets, then the
  // sources' offsets (points, tets, node entries, face entries), the table
  // coming back, the sources' descriptors
  const size_t o_x = 0, o_s = o_x + pmx_call::al256((size_t)HP * 24),
               o_t = o_s + pmx_call::al256((size_t)HP * std::max(S, 1) * 8), o_n = o_t + pmx_call::al256((size_t)HT * 16),
               o_f = o_n + pmx_call::al256((size_t)NN * 8), o_e = o_f + pmx_call::al256((size_t)NF * 12),
               o_o = o_e + pmx_call::al256((size_t)(NEN + NEF) * 4),
               o_u = o_o + pmx_call::al256((size_t)(next_n + 1) * 4), o_r = o_u + pmx_call::al256((size_t)4 * G1 * 4),
               o_d = o_r + pmx_call::al256((size_t)2 * G1 * 4), total = o_d + pmx_call::al256((size_t)ngrp * sizeof(HeldDesc));
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return no("sync");   // the arena may still feed an earlier copy
  char *stg = pmx_hstage(ctx, total);
  if (!stg) return refuse();
  double *hx = (double *)(stg + o_x), *hs = (double *)(stg + o_s);
  int4 *ht = (int4 *)(stg + o_t);
  int *hnp = (int *)(stg + o_n), *hns = hnp + NN;
  int *hft = (int *)(stg + o_f), *hf1 = hft + NF, *hf2 = hf1 + NF;
  int *hen = (int *)(stg + o_e), *hef = hen + NEN, *heo = (int *)(stg + o_o), *hu = (int *)(stg + o_u);
  const int *tab = (const int *)(stg + o_r);
  HeldDesc *hd = (HeldDesc *)(stg + o_d);
  for (int i = 0; i < 2 * G1; i++) {
    hu[i] = (int)uoff[i];
    hu[2 * G1 + i] = (int)eoff[i];
  }
  for (int g = 0; g < ngrp; g++) {
    const pmx_ctx *H = src[g].held;
    hd[g] = H ? HeldDesc{H->d_xyz.p, H->d_sol.p, H->d_tets.p, (int)H->np, 1} : HeldDesc{nullptr, nullptr, nullptr, 0, 0};
  }
  // every holder's stream is done with its group before this one reads it
  std::vector<DevEvent> given((size_t)ngrp);
  for (int g = 0; g < ngrp; g++) {
    pmx_ctx *H = src[g].held;
    if (!H || H == ctx) continue;
    if (!given[g].create(false) || !M.ok(hipEventRecord(given[g], H->stream), "event record") ||
        !M.ok(hipStreamWaitEvent(M.s, given[g], 0), "stream wait"))
      return refuse();
  }
  if (!pmx_create_events(P.ev) || !M.ok(hipEventRecord(P.ev[0], M.s), "event record")) return refuse();
  // marks, scans, the group table
  DevBuf<uint8_t> used, tval;
  DevBuf<int> prank, trank, duoff, dtab;
  DevBuf<HeldDesc> ddesc;
  DevBuf<unsigned> fctl;
  if (!M.fill(used, UP, 0, "memset") || !M.fill(tval, UT, 1, "memset") || !M.fill(fctl, FC_NCTL, 0xff, "memset") ||
      !M.up(duoff, (const int *)hu, 4 * G1, "source offsets") || !M.up(ddesc, (const HeldDesc *)hd, ngrp, "sources") ||
      !pmx_dgrow(ctx, dtab, (size_t)2 * G1))
    return refuse();
  for (int g = 0; g < ngrp; g++)
    if (!src[g].held &&
        !M.ok(hipMemsetAsync(used.p + uoff[g], 1, (size_t)(uoff[g + 1] - uoff[g]), M.s), "memset"))
      return refuse();
  if (!pmx_dgrow(ctx, prank, (size_t)UP + 1) || !pmx_dgrow(ctx, trank, (size_t)UT + 1)) return refuse();
  const HeldTabs ht_{ddesc.p, duoff.p, duoff.p + G1, duoff.p + 2 * G1, duoff.p + 3 * G1, ngrp,
                     used.p, tval.p, prank.p, trank.p};
  if (any_held) hipLaunchKernelGGL(k_mf_mark, dim3(Merge::blocks(UT)), dim3(256), 0, M.s, ht_, UT, fctl.p);
  if (!M.scan(ByteFlag{used.p, UP}, prank, UP, "point scan") || !M.scan(ByteFlag{tval.p, UT}, trank, UT, "tet scan"))
    return refuse();
  hipLaunchKernelGGL(k_mf_table, dim3(Merge::blocks(2 * G1)), dim3(256), 0, M.s, (const int *)prank.p,
                     (const int *)trank.p, (const int *)duoff.p, G1, dtab.p);
  unsigned fc[FC_NCTL];
  if (!M.ok(hipMemcpyAsync(stg + o_r, dtab.p, sizeof(int) * (size_t)2 * G1, hipMemcpyDeviceToHost, M.s), "download") ||
      !M.read_words(fc, (const unsigned *)fctl.p, FC_NCTL))
    return refuse();
  if (!M.ok(hipGetLastError(), "launch")) return refuse();
  if (fc[FC_BADV] != NOGRP) return no("a vertex outside 1..np (group " + std::to_string(fc[FC_BADV]) + ")");
  std::vector<int64_t> off((size_t)GT_ROWS * G1, 0);
  for (int g = 0; g <= ngrp; g++) {
    off[GT_P * G1 + g] = tab[g];
    off[GT_T * G1 + g] = tab[G1 + g];
    off[GT_N * G1 + g] = eoff[g];
    off[GT_F * G1 + g] = eoff[G1 + g];
  }
  for (int g = 0; g < ngrp; g++)
    if (off[GT_P * G1 + g + 1] - off[GT_P * G1 + g] < 1 || off[GT_T * G1 + g + 1] - off[GT_T * G1 + g] < 1)
      return no("every point of the held group is dropped: it has no valid tet (group " + std::to_string(g) + ")");
  const int64_t NP = off[GT_P * G1 + ngrp], T = off[GT_T * G1 + ngrp];
  P.ngrp = ngrp;
  P.next_node = next_n;
  P.sd = sd;
  P.P = NP; P.T = T; P.NN = NN; P.NF = NF; P.NEN = NEN; P.NEF = NEF;
  P.gt.resize(off.size());
  for (size_t i = 0; i < off.size(); i++) P.gt[i] = (int)off[i];
  // the host sources packed as pmx_merge_groups packs them, at their places;
  // a held source's entries range-checked, in its own numbering from 0
  if (!pmx_dgrow(ctx, P.cxyz, (size_t)(3 * NP)) || !pmx_dgrow(ctx, P.csol, (size_t)std::max<int64_t>((int64_t)S * NP, 1)) ||
      !pmx_dgrow(ctx, P.ctet, (size_t)T))
    return refuse();
  int64_t hp = 0, htt = 0;
  for (int g = 0; g < ngrp; g++) {
    const pmx_merge_group &G = src[g].g;
    const pmx_ctx *H = src[g].held;
    const int64_t p0 = off[GT_P * G1 + g], t0 = off[GT_T * G1 + g], n0 = eoff[g], f0 = eoff[G1 + g];
    if (!H) {
      const MergeHostDst d{hx + 3 * hp, hs + (int64_t)S * hp, ht + htt, hnp + n0, hns + n0, hft + f0, hf1 + f0, hf2 + f0, p0, t0};
      if (!M.pack_host_group(G, g, nsol, sd, nitemN, nitemF, d)) return refuse();
      if (!M.ok(hipMemcpyAsync(P.cxyz.p + 3 * p0, d.x, 24 * (size_t)G.np, hipMemcpyHostToDevice, M.s), "points") ||
          (S > 0 && !M.ok(hipMemcpyAsync(P.csol.p + (int64_t)S * p0, d.s, 8 * (size_t)S * (size_t)G.np,
                                         hipMemcpyHostToDevice, M.s), "solutions")) ||
          !M.ok(hipMemcpyAsync(P.ctet.p + t0, d.t, 16 * (size_t)G.ne, hipMemcpyHostToDevice, M.s), "tets"))
        return refuse();
      hp += G.np;
      htt += G.ne;
      continue;
    }
    const MergeHostDst d{nullptr, nullptr, nullptr, hnp + n0, hns + n0, hft + f0, hf1 + f0, hf2 + f0, 0, 0};
    if (!M.pack_entries(G, g, H->np, H->ne, 0, 0, nitemN, nitemF, d)) return refuse();
  }
  if (!M.pack_ext(comm, nitemN, nitemF, NEN, NEF, hen, hef, heo)) return refuse();
  if (!M.up(P.nep, (const int *)hnp, NN, "node entries") || !M.up(P.nes, (const int *)hns, NN, "node entries") ||
      !M.up(P.fet, (const int *)hft, NF, "face entries") || !M.up(P.fe1, (const int *)hf1, NF, "face entries") ||
      !M.up(P.fe2, (const int *)hf2, NF, "face entries") || !M.up(P.extn, (const int *)hen, NEN, "external items") ||
      !M.up(P.extf, (const int *)hef, NEF, "external items") || !M.up(P.eoff, (const int *)heo, next_n + 1, "external offsets"))
    return refuse();
  // the held sources: rows, connectivity and entries through the ranks, one
  // launch each over all sources
  if (any_held) {
    hipLaunchKernelGGL(k_mf_points, dim3(Merge::blocks(UP * (3 + S))), dim3(256), 0, M.s, ht_, UP, S, P.cxyz.p, P.csol.p);
    hipLaunchKernelGGL(k_mf_tets, dim3(Merge::blocks(UT)), dim3(256), 0, M.s, ht_, UT, P.ctet.p);
    if (NN > 0) hipLaunchKernelGGL(k_mf_node_entries, dim3(Merge::blocks(NN)), dim3(256), 0, M.s, ht_, NN, P.nep.p, fctl.p);
    if (NF > 0)
      hipLaunchKernelGGL(k_mf_face_entries, dim3(Merge::blocks(NF)), dim3(256), 0, M.s, ht_, NF, P.fet.p, P.fe1.p, fctl.p);
  }
  if (any_held) {
    if (!M.read_words(fc, (const unsigned *)fctl.p, FC_NCTL)) return refuse();
    if (!M.ok(hipGetLastError(), "launch")) return refuse();
    const unsigned gbad = std::min(fc[FC_DROPN], fc[FC_DROPF]);
    if (gbad != NOGRP)
      return no(std::string(fc[FC_DROPN] == gbad ? "a node entry names a dropped point: no valid tet holds it"
                                                 : "a face entry names a dropped tet (v[0] <= 0)") +
                " (group " + std::to_string(gbad) + ")");
  }
  if (!M.plan(nitemN, nitemF)) return refuse();
  // back to the sources' own numbering
  if (!pmx_dgrow(ctx, P.upmap, (size_t)UP) || !pmx_dgrow(ctx, P.utnew, (size_t)UT)) return refuse();
  {
    const BackArgs pa{used.p, prank.p, P.pmap.p, P.pgrp.p, duoff.p, P.psrc.p, UP, P.upmap.p, P.pold.p};
    hipLaunchKernelGGL(k_mf_back, dim3(Merge::blocks(UP)), dim3(256), 0, M.s, pa);
    const BackArgs ta{tval.p, trank.p, P.tnew.p, P.tgrp.p, duoff.p + G1, nullptr, UT, P.utnew.p, P.told.p};
    hipLaunchKernelGGL(k_mf_back, dim3(Merge::blocks(UT)), dim3(256), 0, M.s, ta);
  }
  if (!M.ok(hipEventRecord(P.ev[1], M.s), "event record") || !M.sync("plan")) return refuse();
  float ms = 0.f;
  if (!M.ok(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]), "event time")) return refuse();
  // the inputs' device copies are not needed again (the marks and ranks are
  // locals: they go with the call)
  P.cxyz.release();
  P.csol.release();
  P.ctet.release();
  P.uoff = uoff;
  ctx->merge_plan_ms = ms;
  if (sizes) {
    sizes->np = P.np;
    sizes->ne = P.ne;
    sizes->nnode = P.nnode;
    sizes->nface = NEF;
  }
  return 1;
}

}  // extern "C"
