// pmx_contig.hip -- partition contiguity of the uploaded group on the device.
//
// pmx_contiguity     <- PMMG_check_grps_contiguity / PMMG_check_part_contiguity
//                       (src/metis_pmmg.c:446-529, 312-392): the face-connected
//                       components of the group, or of each part of a partition
// pmx_fix_contiguity <- PMMG_fix_contiguity_split / _centralized /
//                       PMMG_fix_contiguity (src/moveinterfaces_pmmg.c:377-611
//                       over the lists of :148-299): all but the largest piece
//                       of a colour merged into a neighbouring colour
//
// Semantics: DESIGN.md section 4, "Partition contiguity".  Two parts:
//
// Labelling.  Min-index hooking over the 32-B tet records: every interior face
// (k, nb > k) of equal colour links the two parent trees with atomicMin, the
// larger node's parent towards the smaller node, and carries on with the link
// the atomic displaced, so that a launch loses no connection.  A pass of
// pointer jumping follows.  Parents only ever decrease and stay inside their
// component, so whatever value a lane reads of a parent another workgroup
// wrote in the same launch -- fresh or stale -- is a valid ancestor: staleness
// costs work, never the answer.  Convergence is decided across kernel
// boundaries: a hooking launch that meets no face with two different roots.
// The root of a converged tree is its smallest tet, the head the reference's
// ascending scans find.  Sizes and "open" bits (some neighbour lies in another
// component) are summed per root, one atomic per run of equal roots in a wave,
// and the roots are compacted into the component table.
//
// Fix.  The reference's loop over colours runs on the host over that table:
// which lists exist, their lengths and whether they have a neighbour outside
// come from it.  Only the tet a losing list merges into (its otetra) depends on
// the list's breadth-first order; a replay kernel reruns that order with one
// lane per losing component, up to the first dequeued tet with a foreign
// neighbour, at most `steps` dequeues per launch (its state lives in global
// memory and the host relaunches), and a recolour kernel applies the merges.
// No kernel here waits on another workgroup.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include "pmx_device.h"
#include "pmx_internal.h"

namespace {

#include "pmx_contig_dev.h"   // the control words, cc_find / cc_link, k_cc_init, k_cc_jump

__global__ __launch_bounds__(256) void k_cc_hook(const TetRec *__restrict__ tets, int64_t ne,
                                                 const int *__restrict__ mark, int *par,
                                                 unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne) return;
  const int4 nb4 = reinterpret_cast<const int4 *>(tets)[2 * k + 1];
  const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
  const int c = mark[k];
  // the neighbours' marks as four independent loads (a face that is not
  // looked at reads the tet's own mark)
  int mk[4];
#pragma unroll
  for (int l = 0; l < 4; l++) mk[l] = mark[(nb[l] > k && nb[l] <= ne) ? (int64_t)nb[l] : k];
  int a = -1;
  bool changed = false;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int k1 = nb[l];
    if (k1 <= k || k1 > ne || mk[l] != c) continue;
    if (a < 0) a = cc_find(par, (int)k);
    const int b = cc_find(par, k1);
    if (a == b) continue;
    changed = true;
    cc_link(par, a, b);
    a = a < b ? a : b;
  }
  if (changed) ctl[CC_CHANGED] = 1u;
}

// per root: size and the open bit in sz[root] (zeroed before); ctl[CC_ROOTS] =
// the number of roots.  A few huge components are the normal case, and one
// atomic per wave on the same word is then bound by that word: each thread
// walks CC_SIZE_ITEMS tets 256 apart and keeps a run (root, count, open) in
// registers, which it flushes when the root changes; what is left at the end
// goes out as one atomic per run of equal roots in the wave.
#define CC_SIZE_ITEMS 16
__device__ __forceinline__ void cc_flush(unsigned *sz, int r, unsigned cnt, bool open) {
  atomicAdd(&sz[r], cnt);
  if (open) atomicOr(&sz[r], CC_OPEN_BIT);
}

__global__ __launch_bounds__(256) void k_cc_sizes(const TetRec *__restrict__ tets, int64_t ne,
                                                  const int *__restrict__ par, unsigned *__restrict__ sz,
                                                  unsigned *__restrict__ ctl) {
  const int64_t k0 = (int64_t)blockIdx.x * (256 * CC_SIZE_ITEMS) + threadIdx.x + 1;
  int cur = 0;
  unsigned cnt = 0, nroots = 0;
  bool copen = false;
  for (int i = 0; i < CC_SIZE_ITEMS; i++) {
    const int64_t k = k0 + (int64_t)i * 256;
    if (k > ne) break;
    const int4 nb4 = reinterpret_cast<const int4 *>(tets)[2 * k + 1];
    const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
    const int r = par[k];
    // four independent loads (a missing neighbour reads the tet's own parent):
    // under their conditions the compiler issues them one after the other
    int pn[4];
#pragma unroll
    for (int l = 0; l < 4; l++) pn[l] = par[(nb[l] > 0 && nb[l] <= ne) ? (int64_t)nb[l] : k];
    const bool open = pn[0] != r || pn[1] != r || pn[2] != r || pn[3] != r;
    nroots += r == (int)k;
    if (r != cur) {
      if (cnt) cc_flush(sz, cur, cnt, copen);
      cur = r;
      cnt = 0;
      copen = false;
    }
    cnt++;
    copen = copen || open;
  }
  if (nroots) atomicAdd(&ctl[CC_ROOTS], nroots);
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(cnt != 0);
  while (todo) {                       // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(cur, leader);
    const bool mine = cnt != 0 && cur == r0;
    const unsigned long long m = __ballot(mine), mo = __ballot(mine && copen);
    // the run's tets: a sum over its lanes
    unsigned tot = mine ? cnt : 0u;
    for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d);
    if (lane == leader) cc_flush(sz, r0, tot, mo != 0);
    todo &= ~m;
  }
}

// the component table {head, colour, size, open}, in no particular order
// (the host sorts it); cap entries
__global__ __launch_bounds__(256) void k_cc_table(int64_t ne, const int *__restrict__ par,
                                                  const int *__restrict__ mark, const unsigned *__restrict__ sz,
                                                  int4 *__restrict__ tab, unsigned cap, unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne || par[k] != (int)k) return;
  const unsigned i = atomicAdd(&ctl[CC_ROOTS], 1u);
  if (i >= cap) return;
  const unsigned s = sz[k];
  tab[i] = make_int4((int)k, mark[k], (int)(s & ~CC_OPEN_BIT), (int)(s >> 31));
}

// One lane per losing component i, three int4 per record:
//   rec[3 i]     = {head, colour, queue offset, queue capacity (= size)}
//   rec[3 i + 1] = {cur, ilist, otetra (0: not found yet), mark[otetra]}
//   rec[3 i + 2] = {dequeues so far, stamp id, -, -}
// The list of section 4: tets dequeued in enqueue order, faces 0..3 in order;
// the first dequeued tet with a neighbour of another colour ends it, that
// neighbour is otetra.  At most `steps` dequeues per launch; an unfinished
// lane counts itself in ctl[CC_PENDING].
__global__ __launch_bounds__(64) void k_cc_replay(const TetRec *__restrict__ tets, int64_t ne,
                                                  const int *__restrict__ mark, int *stamp, int *queue, int4 *rec,
                                                  int n, int steps, unsigned *__restrict__ ctl) {
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
    int mk[4];
#pragma unroll
    for (int l = 0; l < 4; l++) mk[l] = (nb[l] > 0 && nb[l] <= ne) ? mark[nb[l]] : c;
    done++;
#pragma unroll
    for (int l = 0; l < 4; l++)
      if (B.z == 0 && nb[l] > 0 && nb[l] <= ne && mk[l] != c) {
        B.z = nb[l];
        B.w = mk[l];
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
  if (B.z == 0 && B.x >= B.y) err = true;         // an open component has a foreign neighbour
  if (err) {
    ctl[CC_RERR] = 1u;
    B.z = -1;
  }
  C.x += done;
  rec[3 * i + 1] = B;
  rec[3 * i + 2] = C;
  if (B.z == 0) atomicAdd(&ctl[CC_PENDING], 1u);
}

// MERGE: the tets of colour c whose root is listed in rc (sorted by head)
// take the listed colour
__global__ __launch_bounds__(256) void k_cc_recolour(int64_t ne, const int *__restrict__ par, int *mark, int c,
                                                     const int2 *__restrict__ rc, int n) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne || mark[k] != c) return;
  const int r = par[k];
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rc[mid].x < r) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n && rc[lo].x == r) mark[k] = rc[lo].y;
}

struct Comp { int head, colour, size, open; };

struct Contig : pmx_call {
  int64_t ne = 0;
  unsigned nb = 0;             // blocks of 256 over the tets 1..ne
  std::vector<Comp> tab;       // sorted by (colour, head)
  int64_t rounds = 0;
  Contig(pmx_ctx *c, const char *w) : pmx_call{c, w, c->stream} {}

  // the refusals shared with pmx_metis_graph, the buffers, the events
  bool begin() {
    if (!ctx->have_bg) return fail("upload a group first");
    if (4 * ctx->ne >= (1LL << 31)) return fail("4 ne >= 2^31 (32-bit idx_t)");
    ne = ctx->ne;
    nb = blocks(ne);
    const size_t n = (size_t)(ne + 1);
    if (!pmx_dgrow(ctx, ctx->d_cpar, n) || !pmx_dgrow(ctx, ctx->d_cmark, n) || !pmx_dgrow(ctx, ctx->d_cstamp, n) ||
        !pmx_dgrow(ctx, ctx->d_cqueue, n) || !pmx_dgrow(ctx, ctx->d_cctl, CC_NCTL))
      return false;
    if (!pmx_create_events(ctx->contig_ev)) return fail("event");
    ctx->contig_label_ms = ctx->contig_replay_ms = 0.0;
    return true;
  }

  bool tic() { return hipEventRecord(ctx->contig_ev[0], s) == hipSuccess || fail("event record"); }
  // after the stream was synchronised
  bool toc_record() { return hipEventRecord(ctx->contig_ev[1], s) == hipSuccess || fail("event record"); }
  bool toc_add(double &ms) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, ctx->contig_ev[0], ctx->contig_ev[1]) != hipSuccess) return fail("event time");
    ms += t;
    return true;
  }
  bool read_ctl(unsigned *h) { return read_words(h, (const unsigned *)ctx->d_cctl.p, CC_NCTL); }

  // marks from the host's part (tet k at k - 1), or one colour
  bool set_marks(const int32_t *part) {
    if (ne == 0) return true;
    const hipError_t e = part ? hipMemcpyAsync(ctx->d_cmark.p + 1, part, sizeof(int) * (size_t)ne,
                                               hipMemcpyHostToDevice, s)
                              : hipMemsetAsync(ctx->d_cmark.p, 0, sizeof(int) * (size_t)(ne + 1), s);
    return e == hipSuccess || fail("marks upload");
  }

  // the components of the current marks into tab (and d_cpar = the labels)
  bool label() {
    unsigned h[CC_NCTL];
    const TetRec *tets = ctx->d_tets.p;
    int *par = ctx->d_cpar.p;
    unsigned *ctl = ctx->d_cctl.p, *sz = (unsigned *)ctx->d_cqueue.p;
    tab.clear();
    if (hipMemsetAsync(ctl, 0, sizeof(unsigned) * CC_NCTL, s) != hipSuccess) return fail("memset");
    if (!tic()) return false;
    hipLaunchKernelGGL(k_cc_init, dim3((unsigned)((ne + 1 + 255) / 256)), dim3(256), 0, s, tets, ne, par, ctl);
    if (!toc_record() || !read_ctl(h) || !toc_add(ctx->contig_label_ms)) return false;
    if (hipGetLastError() != hipSuccess) return fail("init launch");
    if (h[CC_DELETED]) return fail("a deleted tet (v[0] <= 0): the reference wants a packed mesh");
    if (h[CC_BADREC]) return fail("a tet record with a neighbour outside 0..ne");
    if (ne == 0) return true;
    for (int64_t guard = 0;; guard++) {
      if (guard > ne + 1) return fail("the labelling did not converge");
      if (hipMemsetAsync(ctl + CC_CHANGED, 0, sizeof(unsigned), s) != hipSuccess) return fail("memset");
      if (!tic()) return false;
      hipLaunchKernelGGL(k_cc_hook, dim3(nb), dim3(256), 0, s, tets, ne, (const int *)ctx->d_cmark.p, par, ctl);
      hipLaunchKernelGGL(k_cc_jump, dim3(nb), dim3(256), 0, s, ne, par, (const unsigned *)ctl);
      if (!toc_record() || !read_ctl(h) || !toc_add(ctx->contig_label_ms)) return false;
      if (hipGetLastError() != hipSuccess) return fail("hook launch");
      rounds++;
      if (!h[CC_CHANGED]) break;
    }
    if (hipMemsetAsync(sz, 0, sizeof(unsigned) * (size_t)(ne + 1), s) != hipSuccess ||
        hipMemsetAsync(ctl + CC_ROOTS, 0, sizeof(unsigned), s) != hipSuccess)
      return fail("memset");
    if (!tic()) return false;
    hipLaunchKernelGGL(k_cc_sizes, dim3((unsigned)((ne + 256 * CC_SIZE_ITEMS - 1) / (256 * CC_SIZE_ITEMS))), dim3(256),
                       0, s, tets, ne, (const int *)par, sz, ctl);
    if (!toc_record() || !read_ctl(h) || !toc_add(ctx->contig_label_ms)) return false;
    if (hipGetLastError() != hipSuccess) return fail("sizes launch");
    const unsigned nroots = h[CC_ROOTS];
    if (nroots == 0 || (int64_t)nroots > ne) return fail("root count out of range");
    if (!pmx_dgrow(ctx, ctx->d_ctab, (size_t)nroots)) return false;
    if (hipMemsetAsync(ctl + CC_ROOTS, 0, sizeof(unsigned), s) != hipSuccess) return fail("memset");
    if (!tic()) return false;
    hipLaunchKernelGGL(k_cc_table, dim3(nb), dim3(256), 0, s, ne, (const int *)par, (const int *)ctx->d_cmark.p,
                       (const unsigned *)sz, ctx->d_ctab.p, nroots, ctl);
    if (!toc_record()) return false;
    std::vector<int4> raw(nroots);
    if (hipMemcpyAsync(raw.data(), ctx->d_ctab.p, sizeof(int4) * (size_t)nroots, hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        !read_ctl(h) || !toc_add(ctx->contig_label_ms))
      return false;
    if (hipGetLastError() != hipSuccess) return fail("table launch");
    if (h[CC_ROOTS] != nroots) return fail("root count changed between passes");
    tab.resize(nroots);
    for (unsigned i = 0; i < nroots; i++) tab[i] = Comp{raw[i].x, raw[i].y, raw[i].z, raw[i].w};
    std::sort(tab.begin(), tab.end(), [](const Comp &a, const Comp &b) {
      return a.colour != b.colour ? a.colour < b.colour : a.head < b.head;
    });
    return true;
  }
};

}  // namespace

double pmx_contig_kernel_ms(pmx_ctx *ctx, int which) {
  return which == 12 ? ctx->contig_label_ms : ctx->contig_replay_ms;
}

extern "C" {

int pmx_contiguity(pmx_ctx *ctx, const int32_t *part, int32_t nparts, int32_t *counts, int32_t *label,
                   int64_t *ncomp) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Contig L{ctx, "pmx_contiguity"};
  ctx->contig_label_ms = ctx->contig_replay_ms = -1.0;
  if (nparts < 0 || (counts && nparts == 0)) { L.fail("nparts < 0, or counts without parts"); return 0; }
  if (!L.begin() || !L.set_marks(part) || !L.label()) return 0;
  const int64_t ne = L.ne;
  std::vector<int32_t> lab;
  if (label && ne > 0) {
    lab.resize((size_t)ne);
    if (hipMemcpyAsync(lab.data(), ctx->d_cpar.p + 1, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost, L.s) !=
            hipSuccess ||
        hipStreamSynchronize(L.s) != hipSuccess) {
      L.fail("label download");
      return 0;
    }
    std::copy(lab.begin(), lab.end(), label);
  }
  if (counts) {
    std::fill(counts, counts + nparts, 0);
    for (const Comp &c : L.tab)
      if (c.colour >= 0 && c.colour < nparts) counts[c.colour]++;
  }
  if (ncomp) *ncomp = (int64_t)L.tab.size();
  return 1;
}

}  // extern "C"

namespace {

// FIX on the marks in d_cmark (begin() done), colours in the caller's order;
// steps: dequeues per replay launch
int fix_marks(Contig &L, int32_t ncolors, const int32_t *colors, const std::unordered_map<int, int> &place,
              int steps, pmx_contig_stats &S) {
  pmx_ctx *ctx = L.ctx;
  if (!L.label()) return 0;
  const int64_t ne = L.ne;
  hipStream_t s = L.s;
  S = pmx_contig_stats{};
  S.ncomp = (int64_t)L.tab.size();
  if (ne > 0 && hipMemsetAsync(ctx->d_cstamp.p, 0, sizeof(int) * (size_t)(ne + 1), s) != hipSuccess) {
    L.fail("memset");
    return 0;
  }
  int next_id = 1;
  std::unordered_set<int> dirty;
  struct Loser { int head, size; };
  std::vector<Loser> losers;
  std::vector<int4> rec;
  std::vector<int2> rc;
  unsigned h[CC_NCTL];
  for (int ic = 0; ic < ncolors; ic++) {
    const int c = colors ? colors[ic] : ic;
    if (dirty.count(c)) {
      // a merge enlarged or bridged this colour's components
      if (!L.label()) return 0;
      dirty.clear();
      S.relabels++;
    }
    auto lo = std::lower_bound(L.tab.begin(), L.tab.end(), c, [](const Comp &a, int v) { return a.colour < v; });
    auto hi = lo;
    while (hi != L.tab.end() && hi->colour == c) ++hi;
    if (lo == hi) continue;
    // the reference's loop over this colour's lists, heads ascending
    losers.clear();
    const Comp *mainc = &*lo;
    S.counter += mainc->size;
    for (auto it = lo + 1; it != hi; ++it) {
      const Comp *next = &*it;
      S.counter += next->size;
      if (next->size > mainc->size) {
        if (!mainc->open) S.ncannot++;
        else {
          losers.push_back({mainc->head, mainc->size});
          mainc = next;
        }
      } else {
        if (!next->open) S.ncannot++;
        else losers.push_back({next->head, next->size});
      }
    }
    if (losers.empty()) continue;
    const size_t n = losers.size();
    if ((int64_t)next_id + (int64_t)n >= (1LL << 31) - 1) {
      if (hipMemsetAsync(ctx->d_cstamp.p, 0, sizeof(int) * (size_t)(ne + 1), s) != hipSuccess) {
        L.fail("memset");
        return 0;
      }
      next_id = 1;
    }
    rec.assign(3 * n, make_int4(0, 0, 0, 0));
    int64_t off = 0;
    for (size_t i = 0; i < n; i++) {
      rec[3 * i] = make_int4(losers[i].head, c, (int)off, losers[i].size);
      rec[3 * i + 2] = make_int4(0, next_id++, 0, 0);
      off += losers[i].size;
    }
    if (off > ne) { L.fail("losing components larger than the mesh"); return 0; }
    if (!pmx_dgrow(ctx, ctx->d_crec, 3 * n) || !pmx_dgrow(ctx, ctx->d_crecol, n)) return 0;
    if (hipMemcpyAsync(ctx->d_crec.p, rec.data(), sizeof(int4) * 3 * n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      L.fail("replay upload");
      return 0;
    }
    for (;;) {
      if (hipMemsetAsync(ctx->d_cctl.p + CC_PENDING, 0, sizeof(unsigned), s) != hipSuccess) {
        L.fail("memset");
        return 0;
      }
      if (!L.tic()) return 0;
      hipLaunchKernelGGL(k_cc_replay, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s,
                         (const TetRec *)ctx->d_tets.p, ne, (const int *)ctx->d_cmark.p, ctx->d_cstamp.p,
                         ctx->d_cqueue.p, ctx->d_crec.p, (int)n, steps, ctx->d_cctl.p);
      if (!L.toc_record() || !L.read_ctl(h) || !L.toc_add(ctx->contig_replay_ms)) return 0;
      if (hipGetLastError() != hipSuccess) { L.fail("replay launch"); return 0; }
      S.replays++;
      if (h[CC_RERR]) { L.fail("the replay left its component"); return 0; }
      if (!h[CC_PENDING]) break;
    }
    if (hipMemcpyAsync(rec.data(), ctx->d_crec.p, sizeof(int4) * 3 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      L.fail("replay download");
      return 0;
    }
    rc.resize(n);
    for (size_t i = 0; i < n; i++) {
      const int tgt = rec[3 * i + 1].w;
      S.replay_steps += rec[3 * i + 2].x;
      S.nmerged++;
      S.nmerged_tets += losers[i].size;
      // flag[otetra] == 0: otetra's colour has not had its turn (or never has one)
      const auto p = place.find(tgt);
      const bool processed = p != place.end() && p->second < ic;
      if (!processed) S.counter -= losers[i].size;
      if (p != place.end() && p->second > ic) dirty.insert(tgt);
      rc[i] = make_int2(losers[i].head, tgt);
    }
    std::sort(rc.begin(), rc.end(), [](const int2 &a, const int2 &b) { return a.x < b.x; });
    if (hipMemcpyAsync(ctx->d_crecol.p, rc.data(), sizeof(int2) * n, hipMemcpyHostToDevice, s) != hipSuccess) {
      L.fail("recolour upload");
      return 0;
    }
    if (!L.tic()) return 0;
    hipLaunchKernelGGL(k_cc_recolour, dim3(L.nb), dim3(256), 0, s, ne, (const int *)ctx->d_cpar.p, ctx->d_cmark.p,
                       c, (const int2 *)ctx->d_crecol.p, (int)n);
    if (!L.toc_record()) return 0;
    if (hipStreamSynchronize(s) != hipSuccess) { L.fail("recolour"); return 0; }
    if (!L.toc_add(ctx->contig_replay_ms)) return 0;
    if (hipGetLastError() != hipSuccess) { L.fail("recolour launch"); return 0; }
  }
  S.rounds = L.rounds;
  return 1;
}

// colour -> its place in the order; false: a colour listed twice
bool colour_places(int32_t ncolors, const int32_t *colors, std::unordered_map<int, int> &place) {
  for (int i = 0; i < ncolors; i++)
    if (!place.emplace(colors ? colors[i] : i, i).second) return false;
  return true;
}

int replay_steps_of(int64_t replay_steps) {
  return (int)std::min<int64_t>(replay_steps ? replay_steps : CC_DEFAULT_REPLAY_STEPS, 1 << 30);
}

}  // namespace

int pmx_contig_default_replay_steps() { return CC_DEFAULT_REPLAY_STEPS; }

bool pmx_contig_fix_device(pmx_ctx *ctx, const char *who, int *d_mark, int32_t ncolors, const int32_t *colors,
                           int64_t replay_steps, pmx_contig_stats *st) {
  Contig L{ctx, who};
  ctx->contig_label_ms = ctx->contig_replay_ms = -1.0;
  if (ncolors < 0 || replay_steps < 0) return L.fail("ncolors < 0 or replay_steps < 0");
  std::unordered_map<int, int> place;
  if (!colour_places(ncolors, colors, place)) return L.fail("duplicate colours");
  if (!L.begin()) return false;
  const size_t bytes = sizeof(int) * (size_t)(L.ne + 1);
  if (hipMemcpyAsync(ctx->d_cmark.p, d_mark, bytes, hipMemcpyDeviceToDevice, L.s) != hipSuccess)
    return L.fail("marks copy");
  pmx_contig_stats S{};
  if (!fix_marks(L, ncolors, colors, place, replay_steps_of(replay_steps), S)) return false;
  if (hipMemcpyAsync(d_mark, ctx->d_cmark.p, bytes, hipMemcpyDeviceToDevice, L.s) != hipSuccess ||
      hipStreamSynchronize(L.s) != hipSuccess)
    return L.fail("marks copy");
  if (st) *st = S;
  return true;
}

extern "C" {

int pmx_fix_contiguity(pmx_ctx *ctx, int32_t *part, int32_t ncolors, const int32_t *colors, int64_t replay_steps,
                       pmx_contig_stats *st) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  Contig L{ctx, "pmx_fix_contiguity"};
  ctx->contig_label_ms = ctx->contig_replay_ms = -1.0;
  if (!part) { L.fail("part is NULL"); return 0; }
  if (ncolors < 0 || replay_steps < 0) { L.fail("ncolors < 0 or replay_steps < 0"); return 0; }
  std::unordered_map<int, int> place;
  if (!colour_places(ncolors, colors, place)) { L.fail("duplicate colours"); return 0; }
  if (!L.begin() || !L.set_marks(part)) return 0;
  pmx_contig_stats S{};
  if (!fix_marks(L, ncolors, colors, place, replay_steps_of(replay_steps), S)) return 0;
  const int64_t ne = L.ne;
  hipStream_t s = L.s;
  if (ne > 0) {
    std::vector<int32_t> out((size_t)ne);
    if (hipMemcpyAsync(out.data(), ctx->d_cmark.p + 1, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      L.fail("part download");
      return 0;
    }
    std::copy(out.begin(), out.end(), part);
  }
  if (st) *st = S;
  return 1;
}

}  // extern "C"
