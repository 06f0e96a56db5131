// pmx_reduce.hip -- the statistics' reduction across groups and ranks (host
// folds + RCCL; no kernels).
//
// pmx_qual_fold / pmx_len_fold, pmx_*_allreduce <- the reference's MPI_Reduce
//                         with its custom ops (reference src/quality_pmmg.c:
//                         82-144, 265-307, 661-676): one RCCL all-gather of
//                         the per-rank partials, then the reference's
//                         operators folded in rank order
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <cstring>
#include <vector>
#include "pmx_internal.h"

void qual_to_stats(const pmx_qual_part &r, pmx_qual_stats *st) {
  memset(st, 0, sizeof *st);
  st->ne = r.ne; st->np = r.np; st->max = r.max; st->min = r.min; st->avg = r.avg;
  st->iel = r.iel; st->good = r.good; st->med = r.med; st->nrid = r.nrid;
  for (int i = 0; i < 5; i++) st->his[i] = r.his[i];
  st->iel_grp = (int)r.iel_grp;
  st->cpu = 0;
}
void len_to_stats(const pmx_len_part &r, pmx_len_stats *st) {
  memset(st, 0, sizeof *st);
  st->ned = r.ned; st->nullEdge = r.nullEdge; st->avlen = r.avlen; st->lmin = r.lmin; st->lmax = r.lmax;
  st->amin = r.amin; st->bmin = r.bmin; st->amax = r.amax; st->bmax = r.bmax;
  for (int i = 0; i < 9; i++) st->hl[i] = r.hl[i];
  st->cpu_min = st->cpu_max = 0;
}

// one all-gather of each rank's partial (records of `bytes`), on the call's stream
static bool gather_parts(const pmx_call &C, void *comm, int nranks, const void *dev_part, size_t bytes,
                         std::vector<char> &host) {
  pmx_ctx *ctx = C.ctx;
  if (!pmx_dgrow(ctx, ctx->d_gather, (size_t)nranks * bytes / 8 + 1)) return false;
  const ncclResult_t r = ncclAllGather(dev_part, ctx->d_gather.p, bytes / 8, ncclInt64, (ncclComm_t)comm, C.s);
  if (r != ncclSuccess) return C.fail(std::string("ncclAllGather: ") + ncclGetErrorString(r));
  host.resize((size_t)nranks * bytes);
  return C.read_words(host.data(), (const char *)ctx->d_gather.p, host.size(), "all-gather download");
}

extern "C" {

int pmx_qual_fold(const pmx_qual_part *parts, const int *rank, int n, pmx_qual_stats *out) {
  if (!parts || !out || n < 1) return 0;
  // per rank: the groups in order (PMMG_qualhisto's loop, :216-261: sums,
  // strict max, strict min -> first group on ties); then the ranks in order
  // with the reduce operators (:275-306, custom op :82-98: strict min ->
  // lowest rank on ties)
  memset(out, 0, sizeof *out);
  bool first_rank = true;
  int i = 0;
  while (i < n) {
    const int r = rank ? rank[i] : i;
    pmx_qual_stats g;
    memset(&g, 0, sizeof g);
    g.max = 0.0;          // reference max = DBL_MIN; every partial's max is >= 0
    g.min = 1.e300;       // DBL_MAX
    int grp = 0;
    const int i0 = i;
    while (i < n && (rank ? rank[i] : i) == r) i++;
    const bool single = i - i0 == 1;          // an already merged rank partial
    for (int j = i0; j < i; j++, grp++) {
      const pmx_qual_part &p = parts[j];
      g.np += p.np; g.ne += p.ne; g.avg += p.avg; g.med += p.med; g.good += p.good; g.nrid += p.nrid;
      if (p.max > g.max) g.max = p.max;
      if (p.ne && p.min < g.min) { g.min = p.min; g.iel = p.iel; g.iel_grp = single ? (int)p.iel_grp : grp; }
      for (int h = 0; h < 5; h++) g.his[h] += p.his[h];
    }
    g.cpu = r;
    if (first_rank) {
      *out = g;
      first_rank = false;
      continue;
    }
    out->np += g.np; out->ne += g.ne; out->avg += g.avg; out->med += g.med; out->good += g.good;
    out->nrid += g.nrid;
    if (g.max > out->max) out->max = g.max;
    if (g.min < out->min) { out->min = g.min; out->iel = g.iel; out->iel_grp = g.iel_grp; out->cpu = g.cpu; }
    for (int h = 0; h < 5; h++) out->his[h] += g.his[h];
  }
  return 1;
}

int pmx_len_fold(const pmx_len_part *parts, int n, pmx_len_stats *out) {
  if (!parts || !out || n < 1) return 0;
  // PMMG_compute_lenStats (:106-144) applied in rank order: sums; a strictly
  // smaller lmin takes lmin, amin/bmin AND amax/bmax (the reference's quirk)
  // and cpu_min; a strictly larger lmax takes lmax, amax/bmax and cpu_max
  len_to_stats(parts[0], out);
  out->cpu_min = out->cpu_max = 0;
  for (int r = 1; r < n; r++) {
    const pmx_len_part &in = parts[r];
    out->avlen += in.avlen;
    out->ned += in.ned;
    out->nullEdge += in.nullEdge;
    for (int j = 0; j < 9; j++) out->hl[j] += in.hl[j];
    if (in.lmin < out->lmin) {
      out->lmin = in.lmin; out->amin = in.amin; out->bmin = in.bmin;
      out->amax = in.amax; out->bmax = in.bmax; out->cpu_min = r;
    }
    if (in.lmax > out->lmax) {
      out->lmax = in.lmax; out->amax = in.amax; out->bmax = in.bmax; out->cpu_max = r;
    }
  }
  return 1;
}

int pmx_comm_unique_id(char *id, int len) {
  if (!id || len < (int)sizeof(ncclUniqueId)) return 0;
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return 0;
  memcpy(id, &u, sizeof u);
  return (int)sizeof u;
}

int pmx_comm_init(pmx_ctx *ctx, void **comm, int nranks, const char *id, int rank) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_comm_init", ctx->stream};
  if (!comm || !id || nranks < 1 || rank < 0 || rank >= nranks)
    return C.fail("NULL argument or rank outside 0 .. nranks - 1");
  hipSetDevice(ctx->device);
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  ncclComm_t c;
  const ncclResult_t r = ncclCommInitRank(&c, nranks, u, rank);
  if (r != ncclSuccess) return C.fail(std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  *comm = (void *)c;
  return 1;
}

int pmx_comm_destroy(void *comm) {
  if (!comm) return 0;
  return ncclCommDestroy((ncclComm_t)comm) == ncclSuccess ? 1 : 0;
}

int pmx_qualhisto_allreduce(pmx_ctx *ctx, void *comm, int nranks, const void *dev_parts, int ngrp,
                            pmx_qual_stats *out) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_qualhisto_allreduce", ctx->stream};
  if (!comm || !dev_parts || !out || nranks < 1 || ngrp < 1)
    return C.fail("NULL argument, nranks < 1 or ngrp < 1");
  hipSetDevice(ctx->device);
  // the rank's groups merged first (PMMG_qualhisto's group loop), then one
  // record per rank all-gathered
  std::vector<pmx_qual_part> g((size_t)ngrp);
  if (!C.read_words(g.data(), (const pmx_qual_part *)dev_parts, g.size(), "download")) return 0;
  pmx_qual_stats m;
  std::vector<int> zero((size_t)ngrp, 0);
  pmx_qual_fold(g.data(), zero.data(), ngrp, &m);
  pmx_qual_part mine;
  mine.avg = m.avg; mine.max = m.max; mine.min = m.min; mine.iel = m.iel; mine.ne = m.ne; mine.np = m.np;
  mine.good = m.good; mine.med = m.med; mine.nrid = m.nrid;
  for (int h = 0; h < 5; h++) mine.his[h] = m.his[h];
  mine.iel_grp = m.iel_grp;
  if (!pmx_dgrow(ctx, ctx->d_pub, 32)) return 0;
  PMX_CK(C, hipMemcpyAsync(ctx->d_pub.p, &mine, sizeof mine, hipMemcpyHostToDevice, C.s));
  std::vector<char> h;
  if (!gather_parts(C, comm, nranks, ctx->d_pub.p, sizeof(pmx_qual_part), h)) return 0;
  return pmx_qual_fold((const pmx_qual_part *)h.data(), nullptr, nranks, out);
}

int pmx_prilen_allreduce(pmx_ctx *ctx, void *comm, int nranks, const void *dev_part, pmx_len_stats *out) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_prilen_allreduce", ctx->stream};
  if (!comm || !dev_part || !out || nranks < 1) return C.fail("NULL argument or nranks < 1");
  hipSetDevice(ctx->device);
  std::vector<char> h;
  if (!gather_parts(C, comm, nranks, dev_part, sizeof(pmx_len_part), h)) return 0;
  return pmx_len_fold((const pmx_len_part *)h.data(), nranks, out);
}

}  // extern "C"
