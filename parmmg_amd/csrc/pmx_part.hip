// pmx_part.hip -- the partition between the displacement's marks (or Metis's
// array) and the split, on the device.
//
// pmx_part_from_marks   <- PMMG_part_getInterfaces (src/moveinterfaces_pmmg.c:1150-1212)
//                          on the live displacement's marks; group_mark is what
//                          PMMG_part_getProcs (:1102-1118) reads off a group's first tet
// pmx_part_upload / _download
//                       <- the host's part[] (Metis's) in and out
// pmx_part_fix          <- PMMG_fix_contiguity_split (:377-523) in place
// pmx_split_groups_part (pmx_split.hip) reads the partition where it lies, as
//                          PMMG_split_grps does right after either (src/grpsplit_pmmg.c:1680-1711)
//
// The kernels stream the marks (ne + 1 ints, tet k at k) in quads of four tets
// 4 j .. 4 j + 3: the marks and the partition both start at a 256-B aligned
// base, so a quad is one 16-B load and one 16-B store.  The quads that hold
// slot 0 or reach past ne -- the head and the tail -- go tet by tet.  The grid
// is capped (PT_MAX_BLOCKS workgroups of 256) and strides over the quads, so
// that a workgroup's staging of the colour table pays for many tets.
//
//   MMG target    one pass: check the mark, part = mark / nprocs.
//   DISTR target  pass 1 checks the marks and flags the used colours, the host
//                 numbers them (pmx_part_pack.h), pass 2 recomputes the colour
//                 and writes part = map[colour]: 12 B per tet.  While the table
//                 has at most PT_LDS_COLOURS entries pass 1 keeps a bitmap in
//                 LDS, flushed with one atomicOr per non-zero word and
//                 workgroup, and pass 2 stages the map in LDS; a larger table
//                 takes plain stores of 1 and plain loads in global memory.
//
// A bad mark raises a count and, by atomicMin, the smallest offending tet: the
// refusal names the same tet on every run.  A mark is split as an unsigned
// number after the test for < 0, so no mark can index below or past a table.
// No kernel waits on another workgroup; the atomics are integer or, min and add.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>
#include "pmx_device.h"
#include "pmx_internal.h"
#include "pmx_part_pack.h"

namespace {

// A colour table of at most this many entries lives in LDS: 512 B of bitmap
// in pass 1, 16 KiB of map in pass 2 -- ten workgroups of pass 2 still fit the
// CU's 160 KiB, more than its 8 resident workgroups of 256 threads.  Beyond it
// the table is read and written in global memory (L2 holds it for a long while).
#define PT_LDS_COLOURS 4096
#define PT_MAX_BLOCKS 2048         // 8 workgroups on each of 256 CUs

enum { PT_NBAD = 0, PT_FIRST = 1, PT_NCTL = 2 };
enum { PT_MMG = 0, PT_USED_LDS, PT_USED_MEM, PT_PACK_LDS, PT_PACK_MEM };

struct PtArgs {
  const int *mark;      // ne + 1, tet k at k
  int *part;            // ne + 1 (not written by pass 1)
  int64_t ne;
  unsigned nprocs, myrank, nold;
  const int *sum;       // DISTR: the colours before each rank's, nprocs + 1
  int *tab;             // DISTR: pass 1 the used flags (a bitmap with LDS, one int each without), pass 2 the map
  int ntab;             // DISTR: colours
  unsigned *ctl;
};

// the colour of mark c (MMG target: the local group), -1: a mark the target refuses
template <int MODE> __device__ __forceinline__ int pt_colour(const PtArgs &a, int c) {
  if (c < 0) return -1;
  const unsigned u = (unsigned)c, q = u / a.nprocs, r = u - q * a.nprocs;
  if (MODE == PT_MMG) return (r == a.myrank && q < a.nold) ? (int)q : -1;
  const unsigned lo = (unsigned)a.sum[r], n = (unsigned)a.sum[r + 1] - lo;
  return q < n ? (int)(lo + q) : -1;
}

// one tet: what part[k] becomes (passes that write it)
template <int MODE> __device__ __forceinline__ int pt_tet(const PtArgs &a, unsigned *lds, int64_t k, int mark) {
  const int c = pt_colour<MODE>(a, mark);
  if (c < 0) {
    if (MODE != PT_PACK_LDS && MODE != PT_PACK_MEM) {
      atomicAdd(&a.ctl[PT_NBAD], 1u);
      atomicMin(&a.ctl[PT_FIRST], (unsigned)k);
    }
    return 0;
  }
  if (MODE == PT_MMG) return c;
  if (MODE == PT_USED_LDS) {
    // most tets of a wave carry a colour that is already flagged: look first
    const unsigned bit = 1u << (c & 31);
    if (!(lds[c >> 5] & bit)) atomicOr(&lds[c >> 5], bit);
    return 0;
  }
  if (MODE == PT_USED_MEM) {
    if (a.tab[c] == 0) a.tab[c] = 1;
    return 0;
  }
  if (MODE == PT_PACK_LDS) return (int)lds[c];
  return a.tab[c];
}

template <int MODE> __global__ __launch_bounds__(256) void k_pt(PtArgs a) {
  extern __shared__ __align__(16) unsigned lds[];
  constexpr bool writes = MODE == PT_MMG || MODE == PT_PACK_LDS || MODE == PT_PACK_MEM;
  const int tid = threadIdx.x;
  const int nwords = (a.ntab + 31) >> 5;
  if (MODE == PT_USED_LDS) {
    for (int i = tid; i < nwords; i += 256) lds[i] = 0u;
    __syncthreads();
  }
  if (MODE == PT_PACK_LDS) {
    for (int i = tid; i < a.ntab; i += 256) lds[i] = (unsigned)a.tab[i];
    __syncthreads();
  }
  const int64_t nquad = a.ne / 4 + 1;           // quads 0 .. ne / 4 hold the slots 0 .. ne
  for (int64_t j = (int64_t)blockIdx.x * 256 + tid; j < nquad; j += (int64_t)gridDim.x * 256) {
    const int64_t k0 = 4 * j;
    if (j >= 1 && k0 + 3 <= a.ne) {
      const int4 m = *reinterpret_cast<const int4 *>(a.mark + k0);
      int4 o;
      o.x = pt_tet<MODE>(a, lds, k0, m.x);
      o.y = pt_tet<MODE>(a, lds, k0 + 1, m.y);
      o.z = pt_tet<MODE>(a, lds, k0 + 2, m.z);
      o.w = pt_tet<MODE>(a, lds, k0 + 3, m.w);
      if (writes) *reinterpret_cast<int4 *>(a.part + k0) = o;
    } else {
      // the head (slot 0 is no tet) and the tail
      const int64_t hi = k0 + 3 < a.ne ? k0 + 3 : a.ne;
      for (int64_t k = k0 > 1 ? k0 : 1; k <= hi; k++) {
        const int o = pt_tet<MODE>(a, lds, k, a.mark[k]);
        if (writes) a.part[k] = o;
      }
    }
  }
  if (MODE == PT_USED_LDS) {
    __syncthreads();
    for (int i = tid; i < nwords; i += 256)
      if (lds[i]) atomicOr(reinterpret_cast<unsigned *>(a.tab) + i, lds[i]);
  }
}

// a host partition's values lie in 0..ngrp-1 (k_sp_check's test, before the split is asked)
__global__ __launch_bounds__(256) void k_pt_range(const int *__restrict__ part, int64_t ne, int ngrp,
                                                  unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne) return;
  const int g = part[k];
  if (g < 0 || g >= ngrp) {
    atomicAdd(&ctl[PT_NBAD], 1u);
    atomicMin(&ctl[PT_FIRST], (unsigned)k);
  }
}

struct Part : pmx_call {
  pmx_partition &P;
  Part(pmx_ctx *c, const char *w) : pmx_call{c, w, c->stream}, P(c->partition) {}
  bool held() { return (P.valid && ctx->have_bg) || fail("no partition: call pmx_part_from_marks or pmx_part_upload"); }
  bool zero_ctl() {
    const unsigned h[PT_NCTL] = {0u, 0xffffffffu};
    return grow(P.ctl, PT_NCTL) && ok(hipMemcpyAsync(P.ctl.p, h, sizeof h, hipMemcpyHostToDevice, s), "control words") &&
           sync("control words");
  }
  bool read_ctl(unsigned *h, const char *what) {
    return read_words(h, (const unsigned *)P.ctl.p, PT_NCTL) && ok(hipGetLastError(), what);
  }
  static unsigned quad_blocks(int64_t ne) { return std::min<unsigned>(blocks(ne / 4 + 1), PT_MAX_BLOCKS); }
  template <int MODE> void launch(const PtArgs &a, size_t lds_bytes) {
    hipLaunchKernelGGL(k_pt<MODE>, dim3(quad_blocks(a.ne)), dim3(256), lds_bytes, s, a);
  }
  bool elapsed(double *ms) {
    float t = 0.f;
    if (!ok(hipEventRecord(P.ev[1], s), "event record") || !sync("kernels") ||
        !ok(hipEventElapsedTime(&t, P.ev[0], P.ev[1]), "event time"))
      return false;
    if (ms) *ms = t;
    return true;
  }
  // the partition a call built in P.next becomes the held one
  void install(int ngrp) {
    P.part.swap(P.next);
    P.ngrp = ngrp;
    P.valid = true;
  }
};

}  // namespace

double pmx_part_kernel_ms(pmx_ctx *ctx) { return ctx->partition.valid ? ctx->partition.ms : -1.0; }

void pmx_part_drop(pmx_ctx *ctx) {
  pmx_partition &P = ctx->partition;
  P.valid = false;
  P.ngrp = 0;
  P.group_mark.clear();
  P.ms = -1.0;
}

bool pmx_part_held(pmx_ctx *ctx, const int **part, int *ngrp) {
  const pmx_partition &P = ctx->partition;
  if (!P.valid || !ctx->have_bg) return false;
  *part = P.part.p;
  *ngrp = P.ngrp;
  return true;
}

bool pmx_part_of_marks(pmx_ctx *ctx, const char *who, int target, const int *ngrps_all, DevBuf<int> &dst, int *ngrp,
                       std::vector<int> &group_mark, double *ms) {
  Part L{ctx, who};
  pmx_partition &P = L.P;
  MoveIfcMarks M{};
  if (!pmx_moveifc_live_marks(ctx, &M)) return L.fail("no displacement: call pmx_moveifc_begin");
  if (target != PMX_GRPSPL_DISTR_TARGET && target != PMX_GRPSPL_MMG_TARGET) return L.fail("unknown target");
  const int64_t ne = M.ne;
  const int nprocs = M.nprocs;
  const bool distr = target == PMX_GRPSPL_DISTR_TARGET;
  std::vector<int64_t> sum((size_t)nprocs + 1, 0);
  if (distr) {
    for (int r = 0; r < nprocs; r++) {
      const int n = ngrps_all ? ngrps_all[r] : M.displs[r + 1] - M.displs[r];
      if (n < 0) return L.fail("ngrps_all < 0");
      sum[(size_t)r + 1] = sum[(size_t)r] + n;
    }
    if (sum[(size_t)nprocs] >= (1LL << 31)) return L.fail("the ranks' groups number >= 2^31");
  }
  const int64_t ntab = sum[(size_t)nprocs];
  const bool in_lds = ntab <= PT_LDS_COLOURS;
  const size_t nsum = (size_t)nprocs + 1;
  // the used flags: a bitmap the workgroups' LDS copies are or-ed into, or one int per colour
  const size_t nflag = in_lds ? (size_t)((ntab + 31) / 32) : (size_t)ntab;
  if (!L.grow(dst, (size_t)ne + 1) || (distr && !L.grow(P.tab, nsum + (size_t)std::max<int64_t>(ntab, 1))))
    return false;
  if (!pmx_create_events(P.ev)) return L.fail("event");
  if (((uintptr_t)M.mark | (uintptr_t)dst.p) & 15) return L.fail("a device array off its 16-B alignment");
  if (!L.grow(P.ctl, PT_NCTL) || !L.ok(hipEventRecord(P.ev[0], L.s), "event record") || !L.zero_ctl()) return false;
  PtArgs a{M.mark, dst.p, ne, (unsigned)nprocs, (unsigned)M.myrank, (unsigned)M.nold, nullptr, nullptr, (int)ntab, P.ctl.p};
  unsigned h[PT_NCTL];
  if (!distr) {
    L.launch<PT_MMG>(a, 0);
    if (!L.read_ctl(h, "launch")) return false;
    if (h[PT_NBAD])
      return L.fail("a mark of another rank's group (PMMG_GRPSPL_MMG_TARGET wants local marks): tet " +
                    std::to_string(h[PT_FIRST]) + " is the first of " + std::to_string(h[PT_NBAD]));
    if (!L.elapsed(ms)) return false;
    group_mark.resize((size_t)M.nold);
    for (int g = 0; g < M.nold; g++) group_mark[(size_t)g] = nprocs * g + M.myrank;
    *ngrp = M.nold;
    return true;
  }
  // the table crosses PCIe through the pinned arena: sum up, the flags down, the map up
  int *stage = (int *)pmx_hstage(ctx, sizeof(int) * std::max(nsum, (size_t)std::max<int64_t>(ntab, 1)));
  if (!stage) return false;
  for (size_t r = 0; r < nsum; r++) stage[r] = (int)sum[r];
  a.sum = P.tab.p;
  a.tab = P.tab.p + nsum;
  if (!L.ok(hipMemcpyAsync(P.tab.p, stage, sizeof(int) * nsum, hipMemcpyHostToDevice, L.s), "table upload") ||
      !L.ok(hipMemsetAsync(a.tab, 0, sizeof(int) * std::max<size_t>(nflag, 1), L.s), "memset"))
    return false;
  if (in_lds) L.launch<PT_USED_LDS>(a, sizeof(unsigned) * std::max<size_t>(nflag, 1));
  else L.launch<PT_USED_MEM>(a, 0);
  if (!L.read_ctl(h, "launch")) return false;         // the stream is drained: stage is free again
  if (h[PT_NBAD])
    return L.fail("a mark of no group: tet " + std::to_string(h[PT_FIRST]) + " is the first of " +
                  std::to_string(h[PT_NBAD]));
  if (nflag > 0 && !L.read_words(stage, (const int *)a.tab, nflag, "used colours")) return false;
  std::vector<unsigned char> used((size_t)ntab);
  for (int64_t c = 0; c < ntab; c++)
    used[(size_t)c] = in_lds ? (((const unsigned *)stage)[c >> 5] >> (c & 31)) & 1u : stage[c] != 0;
  std::vector<int> gm((size_t)ntab);
  const int count = pmx_part_pack_map(nprocs, M.myrank, sum.data(), used.data(), stage, gm.data());
  if (ntab > 0 && !L.ok(hipMemcpyAsync(a.tab, stage, sizeof(int) * (size_t)ntab, hipMemcpyHostToDevice, L.s), "map upload"))
    return false;
  if (in_lds) L.launch<PT_PACK_LDS>(a, sizeof(unsigned) * (size_t)std::max<int64_t>(ntab, 1));
  else L.launch<PT_PACK_MEM>(a, 0);
  if (!L.elapsed(ms) || !L.ok(hipGetLastError(), "launch")) return false;
  gm.resize((size_t)count);
  group_mark.swap(gm);
  *ngrp = count;
  return true;
}

extern "C" {

int pmx_part_from_marks(pmx_ctx *ctx, int target, const int *ngrps_all, int32_t *ngrp, int32_t *group_mark) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Part L{ctx, "pmx_part_from_marks"};
  pmx_partition &P = L.P;
  P.ms = -1.0;
  int n = 0;
  double ms = -1.0;
  std::vector<int> gm;
  if (!pmx_part_of_marks(ctx, L.who, target, ngrps_all, P.next, &n, gm, &ms)) return 0;
  L.install(n);
  P.group_mark.swap(gm);
  P.ms = ms;
  if (ngrp) *ngrp = n;
  if (group_mark) std::copy(P.group_mark.begin(), P.group_mark.end(), group_mark);
  return 1;
}

int pmx_part_upload(pmx_ctx *ctx, const int32_t *part, int32_t ngrp) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Part L{ctx, "pmx_part_upload"};
  pmx_partition &P = L.P;
  if (!ctx->have_bg) { L.fail("upload a group first"); return 0; }
  const int64_t ne = ctx->ne;
  if (!part && ne > 0) { L.fail("part is NULL"); return 0; }
  if (ngrp < 1) { L.fail("ngrp < 1"); return 0; }
  if (!L.grow(P.next, (size_t)ne + 1)) return 0;
  if (ne > 0) {
    // through the pinned arena, as every upload of size ne
    int32_t *h = (int32_t *)pmx_hstage(ctx, sizeof(int32_t) * (size_t)ne);
    if (!h) return 0;
    par_for(0, ne, [&](int64_t a, int64_t b) { std::copy(part + a, part + b, h + a); });
    if (!L.zero_ctl()) return 0;
    PMX_CK(L, hipMemcpyAsync(P.next.p + 1, h, sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice, L.s));
    hipLaunchKernelGGL(k_pt_range, dim3(L.blocks(ne)), dim3(256), 0, L.s, (const int *)P.next.p, ne, ngrp, P.ctl.p);
    unsigned c[PT_NCTL];
    if (!L.read_ctl(c, "launch")) return 0;
    if (c[PT_NBAD]) {
      L.fail("a part value outside 0..ngrp-1: tet " + std::to_string(c[PT_FIRST]) + " is the first of " +
             std::to_string(c[PT_NBAD]));
      return 0;
    }
  }
  L.install(ngrp);
  P.group_mark.clear();                 // pmx_part_from_marks is its only source
  P.ms = -1.0;
  return 1;
}

int pmx_part_download(pmx_ctx *ctx, int32_t *part, int32_t *ngrp) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Part L{ctx, "pmx_part_download"};
  if (!L.held()) return 0;
  const int64_t ne = ctx->ne;
  if (part && ne > 0) {
    // the caller's array is written only after the copy succeeded
    const int32_t *h = (const int32_t *)pmx_hstage(ctx, sizeof(int32_t) * (size_t)ne);
    if (!h) return 0;
    if (!L.ok(hipMemcpyAsync((void *)h, L.P.part.p + 1, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost, L.s),
              "part download") ||
        !L.sync("part download"))
      return 0;
    par_for(0, ne, [&](int64_t a, int64_t b) { std::copy(h + a, h + b, part + a); });
  }
  if (ngrp) *ngrp = L.P.ngrp;
  return 1;
}

int pmx_part_fix(pmx_ctx *ctx, int64_t replay_steps, pmx_contig_stats *st) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Part L{ctx, "pmx_part_fix"};
  ctx->contig_label_ms = ctx->contig_replay_ms = -1.0;
  if (!L.held()) return 0;
  // the colours 0..ngrp-1 in that order; the partition changes only when the fix succeeded
  return pmx_contig_fix_device(ctx, L.who, L.P.part.p, L.P.ngrp, nullptr, replay_steps, st) ? 1 : 0;
}

int pmx_part_release(pmx_ctx *ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  pmx_part_drop(ctx);
  pmx_partition &P = ctx->partition;
  P.part.release();
  P.next.release();
  P.tab.release();
  P.ctl.release();
  return 1;
}

}  // extern "C"
