// pmx_seq.hip -- PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME: the reference's
// sequential semantics on top of a step's results, on gfx950.  The visit
// order's kernels and the host code that drives both halves; the walks
// themselves are pmx_bdy.hip's (surface) and pmx_walk.hip's (volume).
//
// The reference runs the surface queries one after the other
// (src/interpmesh_pmmg.c:535-599): in the vertex loop's first-visit order
// through the new tets, each PMMG_locatePointBdy starting from the previous
// one's tria (ifoundTria, :529/:556), with mesh->base counting every locate
// (volume and surface, :521, src/locate_pmmg.c:607/805) and the point flags
// of the shadow tests kept from query to query (PMMG_locatePointInCone marks
// the apex with the base and its scanned neighbours with the apex index, and
// skips a neighbour already marked with it, src/locate_pmmg.c:219,247-249;
// PMMG_locatePointInWedge marks an edge end, :318-323).  A query reads those
// flags only through a wedge test (a walk that meets an already visited
// tria, :640-660).  On the device:
//  1. first-visit keys 4 k + l of every point (k_seq_keys), sorted: the visit
//     order; a scan gives each located point its mesh->base and each
//     surface point its position in the surface sequence;
//  2. a speculative pass of every surface query (the step's walks) starting
//     from the device-semantics result of its predecessor, with its
//     reference base; it records whether the walk ran a wedge test;
//  3. one wavefront replays the sequence (k_seq_resolve): a query whose
//     speculative start is the true one (the previous query's true tria) and
//     whose walk never met the shadow tests keeps its speculative result --
//     it read no carried state; any other is run again by one lane on the
//     reference's own state (tria flags vs base, point flags kept across
//     queries), in order.  A replayed walk that ends stuck hands its point to
//     the exhaustive scan (k_exh_bdy, one launch from the host) and the
//     replay resumes after it.
// The volume half is the same three stages on the volume sequence, with the
// kernels of pmx_walk.hip (launch_seqv_*) and the one-point k_fallback as the
// rescue of a stuck walk.
#include "pmx_device.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"
#include <algorithm>

// the first visit of every new point by the reference's vertex loop: key
// 4 k + l over the valid tets that hold it (atomicMin).  A lane skips the
// vertices its left neighbour (the previous tet) holds: that tet's keys are
// smaller, so the run's leftmost lane gives the minimum (as k_mark_new_tets)
__global__ __launch_bounds__(256) void k_seq_keys(const int4 *__restrict__ tv, int64_t ne,
                                                  unsigned *__restrict__ key) {
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  const int64_t nit = (ne + st - 1) / st;
  const bool lane0 = (threadIdx.x & 63) == 0;
  for (int64_t it = 0; it < nit; it++) {
    const int64_t k = 1 + it * st + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int4 a = k <= ne ? tv[k] : make_int4(0, 0, 0, 0);
    int4 u;
    u.x = __shfl_up(a.x, 1, 64); u.y = __shfl_up(a.y, 1, 64);
    u.z = __shfl_up(a.z, 1, 64); u.w = __shfl_up(a.w, 1, 64);
    if (lane0 || u.x <= 0) u = make_int4(0, 0, 0, 0);
    if (a.x <= 0) continue;
    const int w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int q = w[l];
      if (q != u.x && q != u.y && q != u.z && q != u.w) atomicMin(key + (q - 1), (unsigned)(4 * k + l));
    }
  }
}
// idx[i] = i; the speculative start (1) and base (0) of every point: a
// surface point the loop never reaches (an orphan, located by a step without
// the marks and reset afterwards) walks from tria 1
__global__ __launch_bounds__(256) void k_seq_iota(int *__restrict__ idx, int *__restrict__ sstart,
                                                  int *__restrict__ sbase, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    idx[i] = (int)i;
    sstart[i] = 1;
    sbase[i] = 0;
  }
}
// per visit-order rank: located (a volume or surface point the loop reaches:
// not NUL, not frozen) in the low word, surface in the high word
__global__ __launch_bounds__(256) void k_seq_flags(const unsigned *__restrict__ skey, const int *__restrict__ sidx,
                                                   const int8_t *__restrict__ kind, int64_t n,
                                                   unsigned long long *__restrict__ val) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int8_t kd = kind[sidx[r]];
    const bool loc = skey[r] != 0xffffffffu && (kd == KIND_VOL || kd == KIND_BDY);
    val[r] = (unsigned long long)(loc ? 1u : 0u) | ((unsigned long long)(loc && kd == KIND_BDY ? 1u : 0u) << 32);
  }
}
// mesh->base of each located point (1 + the locates before it), the surface
// and the volume sequences; their lengths into nseq[0] / nseq[1]
__global__ __launch_bounds__(256) void k_seq_assign(const int *__restrict__ sidx,
                                                    const unsigned long long *__restrict__ val,
                                                    const unsigned long long *__restrict__ pre, int64_t n,
                                                    int *__restrict__ base, int *__restrict__ seq,
                                                    int *__restrict__ vseq, int *__restrict__ nseq) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long v = val[r], q = pre[r];
    const unsigned located = (unsigned)(q & 0xffffffffull), bdy = (unsigned)(q >> 32);
    if (v & 1ull) {
      const int i = sidx[r];
      base[i] = (int)located + 1;
      if (v >> 32) seq[bdy] = i;
      else vseq[located - bdy] = i;
    }
    if (r == n - 1) {
      const unsigned long long e = q + v;
      nseq[0] = (int)(e >> 32);
      nseq[1] = (int)((e & 0xffffffffull) - (e >> 32));
    }
  }
}
// the speculative start of every query of a sequence (surface or volume): its
// predecessor's element from the step's (device-semantics) pass; the first
// query starts at element 1 (:529)
__global__ __launch_bounds__(256) void k_seq_starts(const int *__restrict__ seq, const int *__restrict__ nseq,
                                                    const int *__restrict__ elem, int *__restrict__ sstart) {
  const int n = *nseq;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    sstart[seq[j]] = j ? elem[seq[j - 1]] : 1;
}
// flags[j] (j < nmax) = surface position j must be looked at by the replay:
// its speculative walk read carried state (a wedge / cone test) or started
// from another tria than its predecessor's speculative result
__global__ __launch_bounds__(256) void k_seq_sflags(const int *__restrict__ seq, const int *__restrict__ nseq_p,
                                                    const int *__restrict__ sstart, const uint8_t *__restrict__ sw,
                                                    const int *__restrict__ elem, int64_t nmax,
                                                    uint8_t *__restrict__ flags) {
  const int n = *nseq_p;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nmax; j += (int64_t)gridDim.x * blockDim.x) {
    bool bad = false;
    if (j < n) {
      const int i = seq[j];
      const int want = j == 0 ? 1 : elem[seq[j - 1]];
      bad = sw[i] || sstart[i] != want;
    }
    flags[j] = bad ? 1 : 0;
  }
}

// ---- the host side ---------------------------------------------------------------

// The replays' control block on the device: the SEQ_CTL_WORDS words behind
// the four n-sized arrays of d_sqint, cleared by every sequential step
#define SEQ_CTL_WORDS 128
struct SeqCtl {
  // per half: {next position, its start element (-1: the previous point's,
  // after a rescue), state (0 done, 1 stuck: the host rescues the point), the
  // stuck point}
  int surf[4], vol[4];
  int nseq[2];               // sequence lengths: surface, volume (k_seq_assign)
  unsigned nreplay[2];       // replayed queries: surface, volume
  int stk_list, vstk_list;   // the one-point lists of a replayed query that ended stuck
  unsigned stk_count;        // the surface list's count (k_exh_bdy reads it)
  int vfound, vbestk;        // the one-point k_fallback's result words ...
  unsigned vcounts[32];      // ... and its step counters (pmx_kernels.h: PMX_CNT_ERR)
};
static_assert(sizeof(SeqCtl) <= SEQ_CTL_WORDS * sizeof(int), "d_sqint leaves SEQ_CTL_WORDS for the control block");

// the step's sequential buffers (n = nq entries each)
struct SeqBufs {
  unsigned *key, *key2;               // first-visit keys; sorted
  int *idx, *idx2;                    // point indices; in visit order
  unsigned long long *val, *pre;      // located | surface per rank; its scan
  int *sbase, *seq, *vseq, *sstart;   // per point mesh->base, the two sequences, per point speculative start
  SeqCtl *ctl;
};
static SeqBufs seq_bufs(pmx_ctx *c) {
  const int64_t n = c->nq;
  int *w = c->d_sqint.p;
  return {c->d_sqkey.p, c->d_sqkey.p + n, c->d_sqidx.p, c->d_sqidx.p + n, c->d_sqval.p, c->d_sqval.p + n,
          w,            w + n,            w + 2 * n,    w + 3 * n,        reinterpret_cast<SeqCtl *>(w + 4 * n)};
}
static unsigned seq_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

// 1. the visit order: each located point's mesh->base, the surface and the
// volume sequence and their lengths (ctl->nseq); the control block cleared
static bool seq_visit_order(const pmx_call &C, const SeqBufs &b) {
  pmx_ctx *c = C.ctx;
  const int64_t n = c->nq;
  const unsigned nbp = seq_blocks(n);
  if (!C.hip(hipMemsetAsync(b.key, 0xff, (size_t)n * sizeof(unsigned), C.s), "memset") ||
      !C.hip(hipMemsetAsync(b.ctl, 0, sizeof(SeqCtl), C.s), "memset"))
    return false;
  hipLaunchKernelGGL(k_seq_keys, dim3(seq_blocks(c->ntets.n)), dim3(256), 0, C.s, (const int4 *)c->ntets.d_v.p,
                     c->ntets.n, b.key);
  hipLaunchKernelGGL(k_seq_iota, dim3(nbp), dim3(256), 0, C.s, b.idx, b.sstart, b.sbase, n);
  if (!C.sort_pairs(c->d_sqtmp, (const unsigned *)b.key, b.key2, (const int *)b.idx, b.idx2, n, 32, "sort"))
    return false;
  hipLaunchKernelGGL(k_seq_flags, dim3(nbp), dim3(256), 0, C.s, (const unsigned *)b.key2, (const int *)b.idx2,
                     (const int8_t *)c->d_kind.p, n, b.val);
  if (!C.exclusive_sum(c->d_sqtmp, (const unsigned long long *)b.val, b.pre, n, "scan")) return false;
  hipLaunchKernelGGL(k_seq_assign, dim3(nbp), dim3(256), 0, C.s, (const int *)b.idx2,
                     (const unsigned long long *)b.val, (const unsigned long long *)b.pre, n, b.sbase, b.seq, b.vseq,
                     b.ctl->nseq);
  return true;
}

// the speculative start of every query of a sequence: its predecessor's element
static void seq_starts(const pmx_call &C, const SeqBufs &b, const int *seq, const int *nseq) {
  hipLaunchKernelGGL(k_seq_starts, dim3(seq_blocks(C.ctx->nq)), dim3(256), 0, C.s, seq, nseq,
                     (const int *)C.ctx->d_elem.p, b.sstart);
}

// a replay's candidates: the positions below n that the half's flag kernel
// (flags(d_sqflag)) marks, in visit order (the selection keeps it): their
// count in d_sqcand[0], the positions behind it
template <class Flags> static bool seq_candidates(const pmx_call &C, int64_t n, Flags flags) {
  pmx_ctx *c = C.ctx;
  if (!C.grow(c->d_sqflag, (size_t)n) || !C.grow(c->d_sqcand, (size_t)n + 1)) return false;
  flags(c->d_sqflag.p);
  return C.select_flagged(c->d_sqtmp, hipcub::CountingInputIterator<int>(0), (const uint8_t *)c->d_sqflag.p,
                          c->d_sqcand.p + 1, (unsigned *)c->d_sqcand.p, n, "select");
}

// a half's control words: the replay goes on at position pos from element
// start (-1: the previous point's)
static bool seq_put_ctl(const pmx_call &C, int *ctl, int pos, int start) {
  const int h[4] = {pos, start, 0, 0};
  return C.hip(hipMemcpyAsync(ctl, h, sizeof h, hipMemcpyHostToDevice, C.s), "ctl");
}

// 3. a half's replay: resolve() runs the sequence until it is done or a
// replayed query ends stuck; rescue() then answers that one point (it is in
// the half's one-point list) and the replay resumes behind it
template <class Resolve, class Rescue>
static bool seq_replay_loop(const pmx_call &C, int *ctl, Resolve resolve, Rescue rescue) {
  for (;;) {
    int h[4];
    resolve();
    if (!C.read_words(h, (const int *)ctl, 4, "ctl")) return false;
    if (h[2] == 0) return true;
    if (!rescue() || !seq_put_ctl(C, ctl, h[0] + 1, -1)) return false;
  }
}

// a replayed volume walk ended stuck: k_fallback on that one point, with
// counters of its own (stuck count 1, no ties, barrier and error words zero)
static bool seq_rescue_vol(const pmx_call &C, const VolArgs &a, SeqCtl *ctl, unsigned long long *best) {
  pmx_ctx *c = C.ctx;
  const unsigned one = 1u;
  const int imax = 0x7fffffff;
  const unsigned long long umax = ~0ull;
  if (!C.hip(hipMemsetAsync(ctl->vcounts, 0, sizeof ctl->vcounts, C.s), "memset") ||
      !C.hip(hipMemcpyAsync(ctl->vcounts, &one, sizeof one, hipMemcpyHostToDevice, C.s), "fallback") ||
      !C.hip(hipMemcpyAsync(&ctl->vfound, &imax, sizeof imax, hipMemcpyHostToDevice, C.s), "fallback") ||
      !C.hip(hipMemcpyAsync(&ctl->vbestk, &imax, sizeof imax, hipMemcpyHostToDevice, C.s), "fallback") ||
      !C.hip(hipMemcpyAsync(best, &umax, sizeof umax, hipMemcpyHostToDevice, C.s), "fallback"))
    return false;
  VolArgs V = a;
  V.stuck_list = &ctl->vstk_list;
  V.stuck_count = ctl->vcounts;
  V.tie_count = ctl->vcounts + 3;
  V.found = &ctl->vfound;
  V.bestk = &ctl->vbestk;
  V.best = best;
  ExhArgs E{};
  E.xyz = c->d_xyz.p; E.tets = c->d_tets.p; E.ne = c->ne; E.q = c->d_qxyz.p;
  E.list = &ctl->vstk_list; E.count = ctl->vcounts; E.found = &ctl->vfound; E.best = best; E.bestk = &ctl->vbestk;
  E.spin_limit = 1L << 26;
  launch_exhaustive(E, V, c->fallback_blocks, C.s);
  unsigned derr = 0;
  if (!C.read_words(&derr, (const unsigned *)ctl->vcounts + PMX_CNT_ERR, 1, "fallback")) return false;
  return !derr || C.fail("the one-point fallback's grid barrier timed out");
}

// the surface half: every query from its predecessor's tria of the step, then
// the replay on the reference's tria and point flags
static bool seq_surface(const pmx_call &C, const VolArgs &a, const SeqBufs &b) {
  pmx_ctx *c = C.ctx;
  SeqCtl *ctl = b.ctl;
  const int64_t n = c->nq_bdy_ub;
  seq_starts(C, b, b.seq, ctl->nseq);
  // 2. the speculative pass: the step's walks, their overflow pass on hashed
  // lists and twice the threads (C3: 82-96 ms of long speculative walks on
  // linear lists)
  BdyArgs B = bdy_args(c, a);
  B.seq_start = b.sstart;
  B.seq_base = b.sbase;
  B.seq_w = c->d_sqw.p;
  const int ovf_threads = 2 * OVF_THREADS;
  const size_t ws_ints = (size_t)ovf_threads * GHS_WS_INTS;
  if (!C.hip(hipMemsetAsync(c->d_counts.p + 1, 0, 2 * sizeof(unsigned), C.s), "memset") ||
      !C.grow(c->d_ows, ws_ints) || !C.hip(hipMemsetAsync(c->d_ows.p, 0, ws_ints * sizeof(int), C.s), "memset"))
    return false;
  launch_bdy_walks(B, c->d_ows.p, C.s, ovf_threads, true);
  // the reference's state: no tria visited, every point flag still the fan size
  if (!C.hip(hipMemsetAsync(c->d_sqtf.p, 0, (size_t)(c->nt + 1) * sizeof(int), C.s), "memset") ||
      !C.hip(hipMemsetAsync(c->d_sqpf.p, PF_INIT & 0xff, (size_t)(c->np + 1) * sizeof(int), C.s), "memset") ||
      !seq_put_ctl(C, ctl->surf, 0, 1))
    return false;
  if (!seq_candidates(C, n, [&](uint8_t *flags) {
        hipLaunchKernelGGL(k_seq_sflags, dim3(seq_blocks(n)), dim3(256), 0, C.s, (const int *)b.seq,
                           (const int *)ctl->nseq, (const int *)b.sstart, (const uint8_t *)c->d_sqw.p,
                           (const int *)c->d_elem.p, n, flags);
      }))
    return false;
  const SeqBdyArgs Q{b.seq,    ctl->nseq,      b.sstart,        b.sbase,      c->d_sqw.p,        c->d_sqtf.p, c->d_sqpf.p,
                     ctl->surf, &ctl->stk_list, &ctl->stk_count, ctl->nreplay, c->d_sqcand.p + 1, c->d_sqcand.p};
  // the rescue: the exhaustive scan of the one-point list
  BdyArgs X = B;
  X.stuck_list = &ctl->stk_list;
  X.stuck_count = &ctl->stk_count;
  return seq_replay_loop(C, ctl->surf, [&] { launch_seq_resolve(B, Q, C.s); },
                         [&] { launch_exh_bdy(X, 1, C.s); return true; });
}

// the volume half: every walk from its predecessor's tet of the step, then
// the replay on the reference's tet flags
static bool seq_volume(const pmx_call &C, const VolArgs &a, const SeqBufs &b) {
  pmx_ctx *c = C.ctx;
  SeqCtl *ctl = b.ctl;
  const int64_t n = c->nq_vol_ub;
  seq_starts(C, b, b.vseq, ctl->nseq + 1);
  SeqVolArgs SV{b.vseq,    ctl->nseq + 1,   b.sstart,         b.sbase, c->d_sqw.p, c->d_sqtv.p,
                ctl->vol,  &ctl->vstk_list, ctl->nreplay + 1, nullptr, nullptr};
  // 2. the speculative pass; its overflow pass's hash tables: generation 0 =
  // empty (positions start at 1)
  if (!C.grow(c->d_sqows, seqv_ovf_ws_ints()) ||
      !C.hip(hipMemsetAsync(c->d_sqows.p, 0, seqv_ovf_ws_ints() * sizeof(int), C.s), "memset"))
    return false;
  launch_seqv_spec(a, SV, n, c->d_sqows.p, C.s);
  // the positions whose speculative start may be wrong
  if (!seq_candidates(C, n, [&](uint8_t *flags) { launch_seqv_flags(a, SV, n, flags, C.s); })) return false;
  SV.ncand = c->d_sqcand.p;
  SV.cand = c->d_sqcand.p + 1;
  // the reference's state: no tet visited
  if (!C.hip(hipMemsetAsync(c->d_sqtv.p, 0, (size_t)(c->ne + 1) * sizeof(int), C.s), "memset") ||
      !seq_put_ctl(C, ctl->vol, 0, 1))
    return false;
  return seq_replay_loop(C, ctl->vol, [&] { launch_seqv_resolve(a, SV, C.s); },
                         [&] { return seq_rescue_vol(C, a, ctl, b.val); });
}

bool pmx_ctx::seq_replay(const VolArgs &a, hipStream_t s, bool surf, bool vol) {
  const pmx_call C{this, "sequential replay", s};
  seq_stats[0] = seq_stats[1] = seq_stats[2] = seq_stats[3] = 0;
  if (!surf && !vol) return true;
  if (!ntets.have)
    return C.fail("PMX_RUN_SEQUENTIAL_*: the first-visit order needs the new tets (points view or pmx_upload_new_tets)");
  if (nq < 1) return true;
  if (!ntets.ensure_tets(s)) return false;
  const size_t n = (size_t)nq;
  if (!C.grow(d_sqkey, 2 * n) || !C.grow(d_sqidx, 2 * n) || !C.grow(d_sqval, 2 * n) ||
      !C.grow(d_sqint, 4 * n + SEQ_CTL_WORDS) || !C.grow(d_sqw, n) ||
      (surf && (!C.grow(d_sqtf, (size_t)(nt + 1)) || !C.grow(d_sqpf, (size_t)(np + 1)))) ||
      (vol && !C.grow(d_sqtv, (size_t)(ne + 1))))
    return false;
  const SeqBufs b = seq_bufs(this);
  if (!seq_visit_order(C, b)) return false;
  if (surf && nq_bdy_ub > 0 && !seq_surface(C, a, b)) return false;
  if (vol && nq_vol_ub > 0 && !seq_volume(C, a, b)) return false;
  unsigned hr[2];
  int hn[2];
  if (!C.hip(hipMemcpyAsync(hr, b.ctl->nreplay, sizeof hr, hipMemcpyDeviceToHost, s), "stats") ||
      !C.read_words(hn, (const int *)b.ctl->nseq, 2, "stats"))
    return false;
  seq_stats[0] = surf ? hr[0] : 0;
  seq_stats[1] = surf ? (unsigned)hn[0] : 0;
  seq_stats[2] = vol ? hr[1] : 0;
  seq_stats[3] = vol ? (unsigned)hn[1] : 0;
  return C.hip(hipGetLastError(), "launch");
}
