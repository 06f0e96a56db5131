// pmx_reach.hip -- reachability of the displaced colours on the device.
//
// pmx_reach_face_marks   <- the marks PMMG_check_reachability puts into the
//                           internal face communicator (src/moveinterfaces_pmmg.c:
//                           664-670); the exchange itself stays with the caller
// pmx_check_reachability <- steps 2 and 3 of PMMG_check_reachability (:724-790
//                           over the lists of :148-299)
// pmx_moveifc_fix / pmx_moveifc_reach
//                        <- the two calls that end PMMG_part_moveInterfaces
//                           (:1446-1452), on the live displacement's marks
//
// Semantics: DESIGN.md section 4, "Reachability".  The state is the marks and
// one flag per tet: after the fix a tet is flagged exactly when its mark is
// one of the rank's colours.
//
// Labelling.  The min-index hooking of pmx_contig.hip, over the faces between
// two unflagged tets of equal mark only; a flagged tet stays its own root.
//
// Reach.  Every entry whose tet is unflagged and has the colour received for
// it marks the root of its component; a tet whose root is marked is flagged.
// The result is a set, so the order of the entries does not matter.
//
// Merge.  The reference's ascending scan runs in rounds on the host over the
// table of the unflagged components: each starts at its smallest tet at or
// above the scan pointer, one lane per component replays its breadth-first
// list up to the first neighbour outside it (at most `steps` dequeues per
// launch, state in global memory, the host relaunches), and the host takes the
// components in ascending start order.  A target that was flagged when the
// round began keeps its mark; a target in a component already taken has that
// component's new mark and is flagged; the first merge into a component not
// yet taken ends the round: what was decided is applied by root, the pointer
// moves behind that start, and the labelling is redone.
// No kernel here waits on another workgroup.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include "pmx_device.h"
#include "pmx_internal.h"

namespace {

#include "pmx_contig_dev.h"   // the control words, cc_find / cc_link, k_cc_init, k_cc_jump

// further control words of this file, behind the shared ones
enum { RC_NSEEDS = 5, RC_NREACHED = 6, RC_LEFT = 7 };   // RC_NSEEDS shares CC_RERR's word: never live together
#define RC_NOSTART 0x7f7f7f7f                           // memset(0x7f): above every tet index

// out[i] = mark[face_index1[i] / 12]
__global__ __launch_bounds__(256) void k_rc_face_marks(int64_t n, const int *__restrict__ fi,
                                                       const int *__restrict__ mark, int *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = mark[fi[i] / 12];
}

// flag[k] = mark[k] is one of the sorted colours col[0..n-1]
__global__ __launch_bounds__(256) void k_rc_flags(int64_t ne, const int *__restrict__ mark,
                                                  const int *__restrict__ col, int n, int *__restrict__ flag) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > ne) return;
  if (k == 0) {
    flag[0] = 1;
    return;
  }
  const int c = mark[k];
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (col[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  flag[k] = lo < n && col[lo] == c;
}

// k_cc_hook between unflagged tets: a face (k, nb > k) links when both are
// unflagged and have the same mark
__global__ __launch_bounds__(256) void k_rc_hook(const TetRec *__restrict__ tets, int64_t ne,
                                                 const int *__restrict__ mark, const int *__restrict__ flag, int *par,
                                                 unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne || flag[k] != 0) return;
  const int4 nb4 = reinterpret_cast<const int4 *>(tets)[2 * k + 1];
  const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
  const int c = mark[k];
  // the neighbours' marks and flags as independent loads (a face that is not
  // looked at reads the tet's own)
  int mk[4], fl[4];
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int64_t j = (nb[l] > k && nb[l] <= ne) ? (int64_t)nb[l] : k;
    mk[l] = mark[j];
    fl[l] = flag[j];
  }
  int a = -1;
  bool changed = false;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int k1 = nb[l];
    if (k1 <= k || k1 > ne || mk[l] != c || fl[l] != 0) continue;
    if (a < 0) a = cc_find(par, (int)k);
    const int b = cc_find(par, k1);
    if (a == b) continue;
    changed = true;
    cc_link(par, a, b);
    a = a < b ? a : b;
  }
  if (changed) ctl[CC_CHANGED] = 1u;
}

// an entry seeds when its tet is unflagged and has the colour received for it:
// seed[root] = 1 (zeroed before); ctl[RC_NSEEDS] counts the entries
__global__ __launch_bounds__(256) void k_rc_seed(int64_t n, const int *__restrict__ fi, const int *__restrict__ cin,
                                                 const int *__restrict__ mark, const int *__restrict__ flag,
                                                 const int *__restrict__ par, int *seed, unsigned *ctl) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ie = fi[i] / 12, c = cin[i];
  if (c == -1 || mark[ie] != c || flag[ie] != 0) return;
  seed[par[ie]] = 1;
  atomicAdd(&ctl[RC_NSEEDS], 1u);
}

// a wave's sum of v into *dst, one atomic
__device__ __forceinline__ void rc_wave_add(unsigned *dst, unsigned v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// flag by root: the tets of a seeded component are flagged.  ctl[RC_NREACHED]
// counts those components, ctl[CC_ROOTS] their tets, ctl[RC_LEFT] the tets
// still unflagged.  No early return: the wave sums want every lane.
__global__ __launch_bounds__(256) void k_rc_reach(int64_t ne, const int *__restrict__ par,
                                                  const int *__restrict__ seed, int *__restrict__ flag,
                                                  unsigned *ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  unsigned hit = 0, root = 0, left = 0;
  if (k <= ne && flag[k] == 0) {
    const int r = par[k];
    if (seed[r]) {
      flag[k] = 1;
      hit = 1;
      root = r == (int)k;
    } else
      left = 1;
  }
  rc_wave_add(&ctl[CC_ROOTS], hit);
  rc_wave_add(&ctl[RC_NREACHED], root);
  rc_wave_add(&ctl[RC_LEFT], left);
}

// per unflagged root: sz[root] = its tets, start[root] = its smallest tet at or
// above the scan pointer `from` (sz zeroed, start RC_NOSTART before);
// ctl[CC_ROOTS] counts the roots.  A wave whose tets share one root sends one
// atomic each.
__global__ __launch_bounds__(256) void k_rc_sizes(int64_t ne, const int *__restrict__ par,
                                                  const int *__restrict__ flag, int from, unsigned *sz, int *start,
                                                  unsigned *ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  const bool on = k <= ne && flag[k] == 0;
  const int r = on ? par[k] : 0;
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(on);
  rc_wave_add(&ctl[CC_ROOTS], on && r == (int)k);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  const int r0 = __shfl(r, leader);
  const bool uniform = __ballot(on && r != r0) == 0;
  int first = (on && k >= from) ? (int)k : RC_NOSTART;
  if (uniform) {
    for (int d = 32; d > 0; d >>= 1) first = min(first, __shfl_xor(first, d));
    if (lane == leader) {
      atomicAdd(&sz[r0], (unsigned)__popcll(m));
      if (first != RC_NOSTART) atomicMin(&start[r0], first);
    }
  } else if (on) {
    atomicAdd(&sz[r], 1u);
    if (first != RC_NOSTART) atomicMin(&start[r], first);
  }
}

// the table of the unflagged components {start, colour, size, root}, in no
// particular order (the host sorts it); cap entries
__global__ __launch_bounds__(256) void k_rc_table(int64_t ne, const int *__restrict__ par,
                                                  const int *__restrict__ flag, const int *__restrict__ mark,
                                                  const unsigned *__restrict__ sz, const int *__restrict__ start,
                                                  int4 *__restrict__ tab, unsigned cap, unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne || flag[k] != 0 || par[k] != (int)k) return;
  const unsigned i = atomicAdd(&ctl[CC_ROOTS], 1u);
  if (i >= cap) return;
  tab[i] = make_int4(start[k], mark[k], (int)sz[k], (int)k);
}

// One lane per component i of the round, three int4 per record:
//   rec[3 i]     = {start, colour, queue offset, queue capacity (= size)}
//   rec[3 i + 1] = {cur, ilist, otetra (0: not found yet, -1: none), mark[otetra]}
//   rec[3 i + 2] = {dequeues so far, stamp id, flag[otetra], par[otetra]}
// The list of section 4 from `start`: tets dequeued in enqueue order, faces
// 0..3 in order; the first dequeued tet with a neighbour outside the list --
// flagged, or of another mark -- ends it, that neighbour is otetra.  A list
// that runs out has none.  At most `steps` dequeues per launch; an unfinished
// lane counts itself in ctl[CC_PENDING].
__global__ __launch_bounds__(64) void k_rc_replay(const TetRec *__restrict__ tets, int64_t ne,
                                                  const int *__restrict__ mark, const int *__restrict__ flag,
                                                  const int *__restrict__ par, int *stamp, int *queue, int4 *rec, int n,
                                                  int steps, unsigned *__restrict__ ctl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int4 A = rec[3 * i];
  int4 B = rec[3 * i + 1], C = rec[3 * i + 2];
  if (B.z != 0) return;
  const int c = A.y, id = C.y;
  int *q = queue + A.z;
  if (B.y == 0) {
    stamp[A.x] = id;
    q[0] = A.x;
    B.y = 1;
  }
  int done = 0;
  bool err = false;
  while (B.x < B.y && done < steps && !err) {
    const int k = q[B.x];
    const int4 nb4 = reinterpret_cast<const int4 *>(tets)[2 * (int64_t)k + 1];
    const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
    int mk[4], fl[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const bool in = nb[l] > 0 && nb[l] <= ne;
      mk[l] = in ? mark[nb[l]] : c;
      fl[l] = in ? flag[nb[l]] : 0;
    }
    done++;
#pragma unroll
    for (int l = 0; l < 4; l++)
      if (B.z == 0 && nb[l] > 0 && nb[l] <= ne && (mk[l] != c || fl[l] != 0)) {
        B.z = nb[l];
        B.w = mk[l];
        C.z = fl[l];
      }
    if (B.z != 0) break;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int k1 = nb[l];
      if (k1 <= 0 || k1 > ne || stamp[k1] == id) continue;
      if (B.y >= A.w) { err = true; break; }     // more tets than the component has: never write past the queue
      stamp[k1] = id;
      q[B.y++] = k1;
    }
    B.x++;
  }
  if (err) {
    ctl[CC_RERR] = 1u;
    B.z = -1;
  } else if (B.z > 0) {
    C.w = par[B.z];
  } else if (B.x >= B.y) {
    B.z = -1;                                      // a component without a neighbour outside
  }
  C.x += done;
  rec[3 * i + 1] = B;
  rec[3 * i + 2] = C;
  if (B.z == 0) atomicAdd(&ctl[CC_PENDING], 1u);
}

// mark and flag by root: an unflagged tet whose root is listed in dec (sorted
// by root) takes {mark, flag} = dec.y, dec.z
__global__ __launch_bounds__(256) void k_rc_apply(int64_t ne, const int *__restrict__ par, int *mark, int *flag,
                                                  const int4 *__restrict__ dec, int n) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne || flag[k] != 0) return;
  const int r = par[k];
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (dec[mid].x < r) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n && dec[lo].x == r) {
    mark[k] = dec[lo].y;
    flag[k] = dec[lo].z;
  }
}

struct RComp { int start, colour, size, root; };

struct Reach : pmx_call {
  int64_t ne = 0;
  unsigned nb = 0;               // blocks of 256 over the tets 1..ne
  int *mark = nullptr, *flag = nullptr, *par = nullptr, *seed = nullptr, *start = nullptr;
  unsigned *sz = nullptr, *ctl = nullptr;
  double ms = 0.0;
  Reach(pmx_ctx *c, const char *w) : pmx_call{c, w, c->stream} {}

  // the refusals every call shares, the buffers, the events
  bool begin(int64_t nface) {
    if (!ctx->have_bg) return fail("upload a group first");
    if (4 * ctx->ne >= (1LL << 31)) return fail("4 ne >= 2^31 (32-bit idx_t)");
    ne = ctx->ne;
    nb = blocks(ne);
    const size_t n = (size_t)(ne + 1);
    if (!grow(ctx->d_cpar, n) || !grow(ctx->d_cmark, n) || !grow(ctx->d_cstamp, n) || !grow(ctx->d_cqueue, n) ||
        !grow(ctx->d_cctl, CC_NCTL) || !grow(ctx->d_rflag, n) || !grow(ctx->d_raux, 3 * n) ||
        !grow(ctx->d_rface, 3 * (size_t)std::max<int64_t>(nface, 1)))
      return false;
    if (!pmx_create_events(ctx->contig_ev)) return fail("event");
    mark = ctx->d_cmark.p;
    flag = ctx->d_rflag.p;
    par = ctx->d_cpar.p;
    seed = ctx->d_raux.p;
    sz = (unsigned *)ctx->d_raux.p + n;
    start = ctx->d_raux.p + 2 * n;
    ctl = ctx->d_cctl.p;
    return true;
  }

  bool tic() { return ok(hipEventRecord(ctx->contig_ev[0], s), "event record"); }
  // the control words down (the stream synchronised), the time since tic() added
  bool toc(unsigned *h) {
    float t = 0.f;
    if (!ok(hipEventRecord(ctx->contig_ev[1], s), "event record") ||
        !read_words(h, (const unsigned *)ctl, (size_t)CC_NCTL) ||
        !ok(hipEventElapsedTime(&t, ctx->contig_ev[0], ctx->contig_ev[1]), "event time"))
      return false;
    ms += t;
    return ok(hipGetLastError(), "kernel launch");
  }

  // the marks into d_cmark: the host's (tet k at k - 1) or a device array (ne + 1 ints)
  bool stage_in(const int32_t *host, const int *dev) {
    if (!ok(hipMemsetAsync(mark, 0, sizeof(int), s), "memset")) return false;
    if (ne == 0) return true;
    return host ? ok(hipMemcpyAsync(mark + 1, host, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, s),
                     "marks upload")
                : ok(hipMemcpyAsync(mark + 1, dev + 1, sizeof(int) * (size_t)ne, hipMemcpyDeviceToDevice, s),
                     "marks copy");
  }

  // the entries onto the device: face_index1, then color_in (may be NULL)
  bool stage_faces(int64_t nface, const int *fi, const int32_t *cin) {
    if (nface == 0) return true;
    int *d = ctx->d_rface.p;
    return ok(hipMemcpyAsync(d, fi, sizeof(int) * (size_t)nface, hipMemcpyHostToDevice, s), "entries upload") &&
           (!cin ||
            ok(hipMemcpyAsync(d + nface, cin, sizeof(int) * (size_t)nface, hipMemcpyHostToDevice, s), "entries upload"));
  }

  // the components of the unflagged tets by mark: d_cpar = the labels
  bool label(bool first) {
    unsigned h[CC_NCTL];
    const TetRec *tets = ctx->d_tets.p;
    if (!ok(hipMemsetAsync(ctl, 0, sizeof(unsigned) * CC_NCTL, s), "memset") || !tic()) return false;
    hipLaunchKernelGGL(k_cc_init, dim3((unsigned)((ne + 1 + 255) / 256)), dim3(256), 0, s, tets, ne, par, ctl);
    if (!toc(h)) return false;
    if (first && h[CC_DELETED]) return fail("a deleted tet (v[0] <= 0): the reference wants a packed mesh");
    if (first && h[CC_BADREC]) return fail("a tet record with a neighbour outside 0..ne");
    if (ne == 0) return true;
    for (int64_t guard = 0;; guard++) {
      if (guard > ne + 1) return fail("the labelling did not converge");
      if (!ok(hipMemsetAsync(ctl + CC_CHANGED, 0, sizeof(unsigned), s), "memset") || !tic()) return false;
      hipLaunchKernelGGL(k_rc_hook, dim3(nb), dim3(256), 0, s, tets, ne, (const int *)mark, (const int *)flag, par,
                         ctl);
      hipLaunchKernelGGL(k_cc_jump, dim3(nb), dim3(256), 0, s, ne, par, (const unsigned *)ctl);
      if (!toc(h)) return false;
      if (!h[CC_CHANGED]) break;
    }
    return true;
  }
};

// Steps 2 and 3 on the marks in d_cmark (begin() and the staging done; the
// entries in d_rface).  colours: the rank's, any order.  counter in / out.
bool reach_marks(Reach &L, const std::vector<int> &colours, int64_t nface, int steps, int64_t &counter,
                 pmx_reach_stats &S) {
  pmx_ctx *ctx = L.ctx;
  hipStream_t s = L.s;
  const int64_t ne = L.ne;
  const size_t n1 = (size_t)(ne + 1);
  const TetRec *tets = ctx->d_tets.p;
  unsigned h[CC_NCTL];
  S = pmx_reach_stats{};
  S.counter = counter;
  // the flags the fix left: a tet is flagged when its mark is a local colour
  std::vector<int> col(colours);
  std::sort(col.begin(), col.end());
  if (!L.grow(ctx->d_rcol, std::max<size_t>(col.size(), 1))) return false;
  if (!col.empty() &&
      !L.ok(hipMemcpyAsync(ctx->d_rcol.p, col.data(), sizeof(int) * col.size(), hipMemcpyHostToDevice, s),
            "colours upload"))
    return false;
  hipLaunchKernelGGL(k_rc_flags, dim3(L.blocks(ne + 1)), dim3(256), 0, s, ne, (const int *)L.mark,
                     (const int *)ctx->d_rcol.p, (int)col.size(), L.flag);
  if (!L.label(true)) return false;
  if (ne == 0) return true;
  // step 2
  if (!L.ok(hipMemsetAsync(L.seed, 0, sizeof(int) * n1, s), "memset") ||
      !L.ok(hipMemsetAsync(L.ctl, 0, sizeof(unsigned) * CC_NCTL, s), "memset") || !L.tic())
    return false;
  if (nface > 0)
    hipLaunchKernelGGL(k_rc_seed, dim3(L.blocks(nface)), dim3(256), 0, s, nface, (const int *)ctx->d_rface.p,
                       (const int *)ctx->d_rface.p + nface, (const int *)L.mark, (const int *)L.flag,
                       (const int *)L.par, L.seed, L.ctl);
  hipLaunchKernelGGL(k_rc_reach, dim3(L.nb), dim3(256), 0, s, ne, (const int *)L.par, (const int *)L.seed, L.flag,
                     L.ctl);
  if (!L.toc(h)) return false;
  S.nseeds = h[RC_NSEEDS];
  S.nreached = h[RC_NREACHED];
  S.nreached_tets = h[CC_ROOTS];
  S.counter += S.nreached_tets;
  if (h[RC_LEFT] == 0) {
    counter = S.counter;
    return true;
  }
  // step 3
  if (!L.ok(hipMemsetAsync(ctx->d_cstamp.p, 0, sizeof(int) * n1, s), "memset")) return false;
  int next_id = 1, from = 1;
  std::vector<int4> raw, rec, dec;
  std::vector<RComp> comps;
  std::unordered_map<int, int> taken;      // root -> the mark it took (and a flag) this round
  for (;;) {
    // the table of what is left
    if (!L.ok(hipMemsetAsync(L.sz, 0, sizeof(unsigned) * n1, s), "memset") ||
        !L.ok(hipMemsetAsync(L.start, 0x7f, sizeof(int) * n1, s), "memset") ||
        !L.ok(hipMemsetAsync(L.ctl, 0, sizeof(unsigned) * CC_NCTL, s), "memset") || !L.tic())
      return false;
    hipLaunchKernelGGL(k_rc_sizes, dim3(L.nb), dim3(256), 0, s, ne, (const int *)L.par, (const int *)L.flag, from,
                       L.sz, L.start, L.ctl);
    if (!L.toc(h)) return false;
    const unsigned nroots = h[CC_ROOTS];
    if ((int64_t)nroots > ne) return L.fail("root count out of range");
    if (nroots == 0) break;
    if (!L.grow(ctx->d_ctab, (size_t)nroots) ||
        !L.ok(hipMemsetAsync(L.ctl + CC_ROOTS, 0, sizeof(unsigned), s), "memset") || !L.tic())
      return false;
    hipLaunchKernelGGL(k_rc_table, dim3(L.nb), dim3(256), 0, s, ne, (const int *)L.par, (const int *)L.flag,
                       (const int *)L.mark, (const unsigned *)L.sz, (const int *)L.start, ctx->d_ctab.p, nroots, L.ctl);
    raw.resize(nroots);
    if (!L.ok(hipMemcpyAsync(raw.data(), ctx->d_ctab.p, sizeof(int4) * (size_t)nroots, hipMemcpyDeviceToHost, s),
              "table download") ||
        !L.toc(h))
      return false;
    if (h[CC_ROOTS] != nroots) return L.fail("root count changed between passes");
    // a component wholly below the pointer is never met again
    comps.clear();
    for (const int4 &r : raw)
      if (r.x != RC_NOSTART) comps.push_back(RComp{r.x, r.y, r.z, r.w});
    if (comps.empty()) break;
    std::sort(comps.begin(), comps.end(), [](const RComp &a, const RComp &b) { return a.start < b.start; });
    S.rounds++;
    // the lists
    const size_t n = comps.size();
    if ((int64_t)next_id + (int64_t)n >= (1LL << 31) - 1) {
      if (!L.ok(hipMemsetAsync(ctx->d_cstamp.p, 0, sizeof(int) * n1, s), "memset")) return false;
      next_id = 1;
    }
    rec.assign(3 * n, make_int4(0, 0, 0, 0));
    int64_t off = 0;
    for (size_t i = 0; i < n; i++) {
      rec[3 * i] = make_int4(comps[i].start, comps[i].colour, (int)off, comps[i].size);
      rec[3 * i + 2] = make_int4(0, next_id++, 0, 0);
      off += comps[i].size;
    }
    if (off > ne) return L.fail("unflagged components larger than the mesh");
    if (!L.grow(ctx->d_crec, 3 * n) || !L.grow(ctx->d_rdec, n) ||
        !L.ok(hipMemcpyAsync(ctx->d_crec.p, rec.data(), sizeof(int4) * 3 * n, hipMemcpyHostToDevice, s),
              "replay upload") ||
        !L.sync("replay upload"))
      return false;
    for (;;) {
      if (!L.ok(hipMemsetAsync(L.ctl + CC_PENDING, 0, sizeof(unsigned), s), "memset") || !L.tic()) return false;
      hipLaunchKernelGGL(k_rc_replay, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, tets, ne, (const int *)L.mark,
                         (const int *)L.flag, (const int *)L.par, ctx->d_cstamp.p, ctx->d_cqueue.p, ctx->d_crec.p,
                         (int)n, steps, L.ctl);
      if (!L.toc(h)) return false;
      S.replays++;
      if (h[CC_RERR]) return L.fail("the replay left its component");
      if (!h[CC_PENDING]) break;
    }
    if (!L.ok(hipMemcpyAsync(rec.data(), ctx->d_crec.p, sizeof(int4) * 3 * n, hipMemcpyDeviceToHost, s),
              "replay download") ||
        !L.sync("replay download"))
      return false;
    // the scan over this round's components, starts ascending
    taken.clear();
    dec.clear();
    bool again = false;
    for (size_t i = 0; i < n && !again; i++) {
      const int4 B = rec[3 * i + 1], C = rec[3 * i + 2];
      const int size = comps[i].size;
      S.replay_steps += C.x;
      S.nunreached++;
      S.counter += size;
      if (B.z < 0) {                                // no neighbour outside: it stays, flagged
        S.ncannot++;
        taken[comps[i].root] = comps[i].colour;
        dec.push_back(make_int4(comps[i].root, comps[i].colour, 1, 0));
        continue;
      }
      int tmark = B.w, tflag = 1;
      if (C.z == 0) {                               // the target was unflagged when the round began
        const auto t = taken.find(C.w);
        if (t != taken.end()) tmark = t->second;
        else tflag = 0;
      }
      S.nmerged++;
      S.nmerged_tets += size;
      dec.push_back(make_int4(comps[i].root, tmark, tflag, 0));
      if (tflag) {
        taken[comps[i].root] = tmark;
      } else {                                      // unflagged again under the new colour: the round ends here
        S.counter -= size;
        S.nrescanned++;
        from = comps[i].start + 1;
        again = true;
      }
    }
    std::sort(dec.begin(), dec.end(), [](const int4 &a, const int4 &b) { return a.x < b.x; });
    if (!L.ok(hipMemcpyAsync(ctx->d_rdec.p, dec.data(), sizeof(int4) * dec.size(), hipMemcpyHostToDevice, s),
              "decisions upload") ||
        !L.tic())
      return false;
    hipLaunchKernelGGL(k_rc_apply, dim3(L.nb), dim3(256), 0, s, ne, (const int *)L.par, L.mark, L.flag,
                       (const int4 *)ctx->d_rdec.p, (int)dec.size());
    if (!L.toc(h)) return false;
    if (!again) break;
    if (!L.label(false)) return false;
    S.relabels++;
  }
  counter = S.counter;
  return true;
}

// nface, the arrays and the entries' tets
bool check_faces(const Reach &L, int64_t ne, int64_t nface, const int *fi, const void *second) {
  if (nface < 0 || (nface > 0 && (!fi || !second))) return L.fail("nface < 0 or a NULL array");
  for (int64_t i = 0; i < nface; i++)
    if (fi[i] / 12 < 1 || fi[i] / 12 > ne) return L.fail("an entry whose tet is outside 1..ne");
  return true;
}

int steps_of(int64_t replay_steps) {
  return (int)std::min<int64_t>(replay_steps ? replay_steps : pmx_contig_default_replay_steps(), 1 << 30);
}

}  // namespace

double pmx_reach_kernel_ms(pmx_ctx *ctx, int which) {
  if (which == 22) return ctx->reach_ms;
  return ctx->moveifc_valid ? ctx->moveifc_fix_ms : -1.0;
}

extern "C" {

int pmx_reach_face_marks(pmx_ctx *ctx, const int32_t *mark, int64_t nface, const int *face_index1, int32_t *out) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Reach L{ctx, "pmx_reach_face_marks"};
  if (!ctx->have_bg) { L.fail("upload a group first"); return 0; }
  if (4 * ctx->ne >= (1LL << 31)) { L.fail("4 ne >= 2^31 (32-bit idx_t)"); return 0; }
  if (!check_faces(L, ctx->ne, nface, face_index1, out)) return 0;
  MoveIfcMarks M{};
  if (!mark && !pmx_moveifc_live_marks(ctx, &M)) {
    L.fail("mark is NULL and no displacement is live: call pmx_moveifc_begin");
    return 0;
  }
  if (nface == 0) return 1;
  // the displacement's marks are read where they live
  if (!L.begin(nface) || (mark && !L.stage_in(mark, nullptr)) || !L.stage_faces(nface, face_index1, nullptr)) return 0;
  int *d = ctx->d_rface.p;
  hipLaunchKernelGGL(k_rc_face_marks, dim3(L.blocks(nface)), dim3(256), 0, L.s, nface, (const int *)d,
                     mark ? (const int *)L.mark : (const int *)M.mark, d + 2 * nface);
  std::vector<int32_t> got((size_t)nface);
  if (!L.read_words(got.data(), (const int32_t *)d + 2 * nface, (size_t)nface, "marks download") ||
      !L.ok(hipGetLastError(), "gather launch"))
    return 0;
  std::copy(got.begin(), got.end(), out);
  return 1;
}

int pmx_check_reachability(pmx_ctx *ctx, int32_t *mark, int32_t ncolors, const int32_t *colors, int64_t nface,
                           const int *face_index1, const int32_t *color_in, int64_t *counter, int64_t replay_steps,
                           pmx_reach_stats *st) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Reach L{ctx, "pmx_check_reachability"};
  ctx->reach_ms = -1.0;
  if (!ctx->have_bg) { L.fail("upload a group first"); return 0; }
  if (4 * ctx->ne >= (1LL << 31)) { L.fail("4 ne >= 2^31 (32-bit idx_t)"); return 0; }
  if (!mark) { L.fail("mark is NULL"); return 0; }
  if (!counter) { L.fail("counter is NULL"); return 0; }
  if (ncolors < 0 || replay_steps < 0) { L.fail("ncolors < 0 or replay_steps < 0"); return 0; }
  std::vector<int> col((size_t)ncolors);
  std::unordered_set<int> seen;
  for (int i = 0; i < ncolors; i++) {
    col[(size_t)i] = colors ? colors[i] : i;
    if (!seen.insert(col[(size_t)i]).second) { L.fail("duplicate colours"); return 0; }
  }
  if (!check_faces(L, ctx->ne, nface, face_index1, color_in)) return 0;
  if (!L.begin(nface) || !L.stage_in(mark, nullptr) || !L.stage_faces(nface, face_index1, color_in)) return 0;
  pmx_reach_stats S{};
  int64_t cnt = *counter;
  if (!reach_marks(L, col, nface, steps_of(replay_steps), cnt, S)) return 0;
  if (L.ne > 0) {
    std::vector<int32_t> got((size_t)L.ne);
    if (!L.read_words(got.data(), (const int32_t *)L.mark + 1, (size_t)L.ne, "marks download")) return 0;
    std::copy(got.begin(), got.end(), mark);
  }
  *counter = cnt;
  if (st) *st = S;
  ctx->reach_ms = L.ms;
  return 1;
}

int pmx_moveifc_fix(pmx_ctx *ctx, int64_t replay_steps, pmx_contig_stats *st) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  pmx_call L{ctx, "pmx_moveifc_fix", ctx->stream};
  ctx->moveifc_fix_ms = -1.0;
  ctx->moveifc_fixed = false;
  MoveIfcMarks M{};
  if (!pmx_moveifc_live_marks(ctx, &M)) { L.fail("no displacement: call pmx_moveifc_begin"); return 0; }
  std::vector<int32_t> col((size_t)M.nold);
  for (int i = 0; i < M.nold; i++) col[(size_t)i] = M.nprocs * i + M.myrank;
  pmx_contig_stats S{};
  if (!pmx_contig_fix_device(ctx, L.who, M.mark, M.nold, col.data(), replay_steps, &S)) return 0;
  ctx->moveifc_fixed = true;
  ctx->moveifc_counter = S.counter;
  ctx->moveifc_fix_ms = ctx->contig_label_ms + ctx->contig_replay_ms;
  if (st) *st = S;
  return 1;
}

int pmx_moveifc_reach(pmx_ctx *ctx, int64_t nface, const int *face_index1, const int32_t *color_in,
                      int64_t replay_steps, pmx_reach_stats *st) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Reach L{ctx, "pmx_moveifc_reach"};
  ctx->reach_ms = -1.0;
  MoveIfcMarks M{};
  if (!pmx_moveifc_live_marks(ctx, &M)) { L.fail("no displacement: call pmx_moveifc_begin"); return 0; }
  if (4 * ctx->ne >= (1LL << 31)) { L.fail("4 ne >= 2^31 (32-bit idx_t)"); return 0; }
  if (!ctx->moveifc_fixed) {
    L.fail("no pmx_moveifc_fix since the last layer or set_colors");
    return 0;
  }
  if (replay_steps < 0) { L.fail("replay_steps < 0"); return 0; }
  if (!check_faces(L, ctx->ne, nface, face_index1, color_in)) return 0;
  std::vector<int> col((size_t)M.nold);
  for (int i = 0; i < M.nold; i++) col[(size_t)i] = M.nprocs * i + M.myrank;
  if (!L.begin(nface) || !L.stage_in(nullptr, M.mark) || !L.stage_faces(nface, face_index1, color_in)) return 0;
  pmx_reach_stats S{};
  int64_t cnt = ctx->moveifc_counter;
  if (!reach_marks(L, col, nface, steps_of(replay_steps), cnt, S)) return 0;
  // the displacement's marks change only now that everything succeeded
  if (L.ne > 0 && (!L.ok(hipMemcpyAsync(M.mark + 1, L.mark + 1, sizeof(int) * (size_t)L.ne, hipMemcpyDeviceToDevice,
                                        L.s),
                         "marks copy") ||
                   !L.sync("marks copy")))
    return 0;
  ctx->moveifc_fixed = false;            // a second check would count the reached lists again
  ctx->moveifc_counter = cnt;
  if (st) *st = S;
  ctx->reach_ms = L.ms;
  return 1;
}

}  // extern "C"
