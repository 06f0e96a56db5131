// pmx_lengths.hip -- edge-length statistics on gfx950.
//
// pmx_prilen[_device]  <- PMMG_prilen / PMMG_computePrilen (reference
//                         src/quality_pmmg.c:370-709): owned parallel edges
//                         first, then every other unique edge in (k, ia)
//                         hash-pop order; the lengths are pmx_metric.h's
// pmx_upload_surface   <- Mmg's surface data (xTetra edge tags, normals,
//                         xPoints) that the tensor lengths are measured along
//
// One pass over the mesh: per-thread accumulation, a wavefront reduction, one
// partial record per workgroup, and a two-level final reduction in workgroup
// order (deterministic sums).  Unique edges are enumerated without a hash
// table: tet k owns its local edge ia iff k is the smallest admissible tet
// index in the edge shell, found by rotating around the edge through the
// adjacency (early exit on the first smaller index) -- the first occurrence
// in the reference's (k ascending, ia ascending) hash-pop order, so endpoints
// and orientation of every length match it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <unordered_set>
#include <vector>
#include "pmx_internal.h"
#include "pmx_metric.h"

#define LEN_STEP2 (1LL << 40)      // keys of tet edges: LEN_STEP2 + 6*k + ia

__constant__ int IARE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

struct LenPart {
  double avlen, lmin, lmax;
  long long kmin, kmax;          // first-occurrence keys of the extremal edges
  long long ned, nul, hl[9];
};

__device__ __forceinline__ int pick_v(const TetRec &t, int l) {
  return (t.v[0] & -(int)(l == 0)) | (t.v[1] & -(int)(l == 1)) | (t.v[2] & -(int)(l == 2)) |
         (t.v[3] & -(int)(l == 3));
}

__device__ __forceinline__ void len_merge(LenPart &x, const LenPart &y) {
  x.avlen += y.avlen;
  if (y.lmin < x.lmin || (y.lmin == x.lmin && y.kmin < x.kmin)) { x.lmin = y.lmin; x.kmin = y.kmin; }
  if (y.lmax > x.lmax || (y.lmax == x.lmax && y.kmax < x.kmax)) { x.lmax = y.lmax; x.kmax = y.kmax; }
  x.ned += y.ned;
  x.nul += y.nul;
  for (int i = 0; i < 9; i++) x.hl[i] += y.hl[i];
}
__device__ __forceinline__ void len_init(LenPart &p) {
  p.avlen = 0.0; p.lmin = 1.e30; p.lmax = 0.0;
  p.kmin = 0x7fffffffffffffffLL; p.kmax = 0x7fffffffffffffffLL;
  p.ned = 0; p.nul = 0;
  for (int i = 0; i < 9; i++) p.hl[i] = 0;
}

__constant__ double BD[9] = {0.0, 0.3, 0.6, 0.7071, 0.9, 1.3, 1.4142, 2.0, 5.0};

// the edge (a, b) is measured elsewhere: an owned parallel edge of step 1 (or,
// exact_once, a parallel edge of another rank).  Sorted (min, max) keys,
// prefiltered by a per-point flag.
__device__ __forceinline__ bool par_excluded(const StatArgs &A, int a, int b) {
  if (!A.npar || !A.par_pt[a] || !A.par_pt[b]) return false;
  const unsigned long long key = ((unsigned long long)(unsigned)min(a, b) << 32) | (unsigned)max(a, b);
  int64_t lo = 0, hi = A.npar;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A.par_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < A.npar && A.par_key[lo] == key;
}

// Edge-length accumulator.  add() is called by every lane of a wave in
// converged control flow ("on" = this lane has an edge).  The histogram and
// the null-edge count are workgroup counters in LDS (one ds_add per edge);
// the sum and the extrema are per lane, reduced in a fixed tree at store().
// (Wave-uniform counters in scalar registers spilled to VGPR lanes: ~900
// readlane/writelane VALU instructions in the loop.)
struct LenAcc {
  unsigned *cnt;                       // LDS [10]: hl[0..8], null edges
  double avlen = 0.0, lmin = 1.e30, lmax = 0.0;
  long long kmin = 0x7fffffffffffffffLL, kmax = 0x7fffffffffffffffLL;
  __device__ explicit LenAcc(unsigned *lds) : cnt(lds) {
    if (threadIdx.x < 10) cnt[threadIdx.x] = 0u;
    __syncthreads();
  }
  __device__ void add(bool on, double len, long long key) {
    if (!on) return;
    if (len == 0.0) { atomicAdd(&cnt[9], 1u); return; }
    // bin i: BD[i] <= len < BD[i+1]; 8: len >= 5, negative or NaN -- the
    // number of bounds BD[1..8] at or below len
    int bin = 0;
#pragma unroll
    for (int i = 1; i < 9; i++) bin += (len >= BD[i]) ? 1 : 0;
    if (!(len >= 0.0)) bin = 8;
    atomicAdd(&cnt[bin], 1u);
    avlen += len;
    if (len < lmin || (len == lmin && key < kmin)) { lmin = len; kmin = key; }
    if (len > lmax || (len == lmax && key < kmax)) { lmax = len; kmax = key; }
  }
  // add() for a lane whose keys strictly increase from call to call (k_prilen:
  // lane t takes ring entry head + t of every round, and the ring is in key
  // order): an equal length never has the smaller key, so the extrema need no
  // key tie-break (the cross-lane tie-breaks stay in store())
  __device__ void add_ordered(bool on, double len, long long key) {
    if (!on) return;
    if (len == 0.0) { atomicAdd(&cnt[9], 1u); return; }
    int bin = 0;
#pragma unroll
    for (int i = 1; i < 9; i++) bin += (len >= BD[i]) ? 1 : 0;
    if (!(len >= 0.0)) bin = 8;
    atomicAdd(&cnt[bin], 1u);
    avlen += len;
    if (len < lmin) { lmin = len; kmin = key; }
    if (len > lmax) { lmax = len; kmax = key; }
  }
  // one LenPart per workgroup: wave shuffles of the per-lane fields, the 4
  // wave results in order, the LDS counters
  __device__ void store(LenPart *out) const {
    __shared__ LenPart wsh[4];
    double s = avlen, lo = lmin, hi = lmax;
    long long klo = kmin, khi = kmax;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double ys = __shfl_xor(s, o, 64), ylo = __shfl_xor(lo, o, 64), yhi = __shfl_xor(hi, o, 64);
      const long long yklo = __shfl_xor(klo, o, 64), ykhi = __shfl_xor(khi, o, 64);
      // the same tree on every lane: the lower lane's value first, so all
      // lanes agree bitwise
      const bool low = (threadIdx.x & o) == 0;
      s = low ? s + ys : ys + s;
      if (ylo < lo || (ylo == lo && yklo < klo)) { lo = ylo; klo = yklo; }
      if (yhi > hi || (yhi == hi && ykhi < khi)) { hi = yhi; khi = ykhi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
      LenPart p;
      p.avlen = s; p.lmin = lo; p.lmax = hi; p.kmin = klo; p.kmax = khi;
      p.ned = 0; p.nul = 0;
      for (int i = 0; i < 9; i++) p.hl[i] = 0;
      wsh[threadIdx.x >> 6] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      LenPart r = wsh[0];
      for (int w = 1; w < (int)(blockDim.x >> 6); w++) len_merge(r, wsh[w]);
      r.ned = 0;
      for (int i = 0; i < 9; i++) { r.hl[i] = cnt[i]; r.ned += cnt[i]; }   // every non-null length has a bin
      r.nul = cnt[9];
      *out = r;
    }
  }
};

// IARE and the two other local vertices of edge ia, as nibble tables (no
// constant-memory load for a per-lane index)
__device__ __forceinline__ int iare0(int ia) { return (0x211000 >> (4 * ia)) & 15; }
__device__ __forceinline__ int iare1(int ia) { return (0x332321 >> (4 * ia)) & 15; }
__device__ __forceinline__ int oth0(int ia) { return (0x000112 >> (4 * ia)) & 15; }
__device__ __forceinline__ int oth1(int ia) { return (0x123233 >> (4 * ia)) & 15; }

__device__ __forceinline__ bool rec_4ridge(const StatArgs &A, const TetRec &t) {
  const int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
  return tet_4ridge(A, v);
}

// One rotation step around the edge (a, b): the shell entered tet r through
// its face (a, b, keep); the next tet is across the face (a, b, w) of r, i.e.
// opposite keep, and w (the sum of r's vertices minus a, b, keep, in modular
// arithmetic) is the vertex of the face crossed next.
__device__ __forceinline__ int rotate_step(const TetRec &r, int a, int b, int &keep) {
  const bool e0 = r.v[0] == keep, e1 = r.v[1] == keep, e2 = r.v[2] == keep;
  const int nb = e0 ? r.nb[0] : e1 ? r.nb[1] : e2 ? r.nb[2] : r.nb[3];
  keep = (int)((unsigned)r.v[0] + (unsigned)r.v[1] + (unsigned)r.v[2] + (unsigned)r.v[3] -
               (unsigned)a - (unsigned)b - (unsigned)keep);
  return nb;
}

// A shell record: from the workgroup's LDS batches when the tet is one of
// them (the current and the previous batch of 256 records: the in-cell and
// x-neighbour shells of a lexicographic numbering), else from HBM.
// L (lean): the batch bases and the tet index in 32-bit arithmetic (tet
// indices < 2^31; the no-batch sentinel is 2^31 modulo 2^32): prilen is
// VALU-bound, and these are on every shell step.
template <bool L>
__device__ __forceinline__ TetRec shell_rec(const StatArgs &A, const TetRec (*srec)[256], long long kb0,
                                            long long kb1, int c) {
  int idx;
  if constexpr (L) {
    const unsigned d0 = (unsigned)c - (unsigned)kb0, d1 = (unsigned)c - (unsigned)kb1;
    idx = d0 < 256u ? (int)d0 : (d1 < 256u ? 256 + (int)d1 : -1);
  } else {
    const unsigned long long d0 = (unsigned long long)((long long)c - kb0);
    const unsigned long long d1 = (unsigned long long)((long long)c - kb1);
    idx = d0 < 256ull ? (int)d0 : (d1 < 256ull ? 256 + (int)d1 : -1);
  }
  // one LDS index into both batches.  The LDS read is unconditional (slot 0
  // for a miss) and only a miss loads from HBM: with both loads conditional
  // the compiler merges them into one flat load through a selected pointer
  // (r06 ISA: flat_load_dwordx4, which waits on both memory counters)
  const int4 *l = reinterpret_cast<const int4 *>(&srec[0][0]) + 2 * (idx < 0 ? 0 : idx);
  int4 lv = l[0], ln = l[1];
  // (opaque to the optimiser: it would otherwise sink the LDS read into the
  // hit branch and merge the two again)
  asm volatile("" : "+v"(lv.x), "+v"(lv.y), "+v"(lv.z), "+v"(lv.w), "+v"(ln.x), "+v"(ln.y), "+v"(ln.z), "+v"(ln.w));
  if (idx < 0) {
    const int4 *g = reinterpret_cast<const int4 *>(A.tets) + 2 * (int64_t)c;
    lv = g[0];
    ln = g[1];
  }
  return TetRec{{lv.x, lv.y, lv.z, lv.w}, {ln.x, ln.y, ln.z, ln.w}};
}

// True iff no admissible tet with index < k contains the edge (a, b) of tet
// k.  The shell is rotated from k through the two faces of k that contain the
// edge (cursors c0, c1; keep0/keep1 = the vertex of the face just crossed),
// both directions advanced together: a smaller index is met after min(d0, d1)
// steps, and a closed shell is covered when the cursors meet.  r0/r1 are the
// records of c0/c1, loaded by the caller (with the edge's points, in one
// round trip) and then one step ahead; without point tags an index alone
// decides, so a record is only loaded when the rotation goes on through it.
template <bool TAGS, bool L>
__device__ __forceinline__ bool owns_edge(const StatArgs &A, const TetRec (*srec)[256], long long kb0, long long kb1,
                                          int64_t k64, int a, int b, int c0, int c1, int keep0, int keep1,
                                          TetRec r0, TetRec r1) {
  using KT = typename std::conditional<L, int, int64_t>::type;
  const KT k = (KT)k64;
  for (int guard = 0; guard < 4096; guard++) {
    if (c0 == (int)k) c0 = 0;                    // a direction that wrapped around
    if (c1 == (int)k) c1 = 0;
    if (!c0 && !c1) return true;                 // both ends reached: every tet seen
    if (!TAGS && ((c0 && c0 < k) || (c1 && c1 < k))) return false;
    if (c0 && c0 == c1) {                        // the cursors meet on one tet
      if (!TAGS) return true;                  // its index was checked above
      return !(c0 < k && !rec_4ridge(A, r0));
    }
    int n0 = 0, n1 = 0;
    if (c0) {
      if (TAGS && c0 < k && !rec_4ridge(A, r0)) return false;
      n0 = rotate_step(r0, a, b, keep0);
    }
    if (c1) {
      if (TAGS && c1 < k && !rec_4ridge(A, r1)) return false;
      n1 = rotate_step(r1, a, b, keep1);
    }
    // closed shell: the next tet of one direction is the one the other just saw
    if (c0 && c1 && (n0 == c1 || n1 == c0)) return true;
    c0 = c0 ? n0 : 0;
    c1 = c1 ? n1 : 0;
    const bool need0 = c0 && c0 != (int)k, need1 = c1 && c1 != (int)k;
    if (!TAGS) {                               // decided by the indices: no load
      if ((need0 && c0 < k) || (need1 && c1 < k)) return false;
      if (need0 && c0 == c1) return true;
    }
    if (need0) r0 = shell_rec<L>(A, srec, kb0, kb1, c0);
    if (need1) r1 = shell_rec<L>(A, srec, kb0, kb1, c1);
  }
  return true;
}

// owns_edge without point tags, as straight-line selects for the first two
// rotation steps (a Kuhn shell of 4 or 6 tets is decided there: the two
// cursors meet), then owns_edge's loop for a longer shell.  The same
// decisions in the same order as owns_edge<false, L>; the loop's early
// returns become a "decided" mask, so the wave issues no branch per check.
// The steps are separate calls so that the caller can put work between them:
// k_prilen evaluates the edge's length while the second step's records load.
template <bool L>
struct FlatRot {
  int c0, c1, keep0, keep1;
  TetRec r0, r1;
  bool done = false, own = true;
  __device__ __forceinline__ void step(const StatArgs &A, const TetRec (*srec)[256], long long kb0, long long kb1,
                                       int64_t k64, int a, int b) {
    using KT = typename std::conditional<L, int, int64_t>::type;
    const KT k = (KT)k64;
    c0 = (c0 == (int)k) ? 0 : c0;
    c1 = (c1 == (int)k) ? 0 : c1;
    // the checks of owns_edge's loop head, first decision wins
    const bool d_end = !c0 && !c1;
    const bool d_small = (c0 && c0 < k) || (c1 && c1 < k);
    const bool d_meet = c0 && c0 == c1;
    own = done ? own : (d_end ? true : (d_small ? false : true));
    done = done || d_end || d_small || d_meet;
    const int n0 = c0 ? rotate_step(r0, a, b, keep0) : 0;
    const int n1 = c1 ? rotate_step(r1, a, b, keep1) : 0;
    const bool d_closed = c0 && c1 && (n0 == c1 || n1 == c0);
    done = done || d_closed;                       // own stays true
    c0 = c0 ? n0 : 0;
    c1 = c1 ? n1 : 0;
    const bool need0 = c0 && c0 != (int)k, need1 = c1 && c1 != (int)k;
    const bool d_small2 = (need0 && c0 < k) || (need1 && c1 < k);
    own = done ? own : !d_small2;
    done = done || d_small2 || (need0 && c0 == c1);
    if (!done && need0) r0 = shell_rec<L>(A, srec, kb0, kb1, c0);
    if (!done && need1) r1 = shell_rec<L>(A, srec, kb0, kb1, c1);
  }
  __device__ __forceinline__ bool finish(const StatArgs &A, const TetRec (*srec)[256], long long kb0, long long kb1,
                                         int64_t k64, int a, int b) {
    if (done) return own;
    return owns_edge<false, L>(A, srec, kb0, kb1, k64, a, b, c0, c1, keep0, keep1, r0, r1);
  }
};

// ---- prilen: unique edges by shell ownership, one pass ------------------------
//
// Each workgroup walks a contiguous range of tets, 256 records per batch:
//  1. every thread reads its tet record (prefetched one batch ahead, kept in a
//     double-buffered LDS array), drops the edges a smaller face neighbour
//     owns (no point tags) and queues the others, in (k, ia) order, in an LDS
//     ring;
//  2. the ring is consumed in full rounds of 256 edges -- one per thread:
//     the edge's points and the first shell step's records are loaded in one
//     round trip, the length is computed, the shell rotation decides whether
//     it counts.  Fewer than 256 left over wait for the next batch, unless
//     they belong to the previous batch, whose LDS records are about to be
//     overwritten (then a partial round).
// (r01 ran the phases as separate launches through a global list: 6.25 ms at
// 125M tets; a fused version with one round trip per dependent load and
// partial rounds after every batch: 7.2 ms.)
#define LEN_QCAP 2048                 // > 255 left over + 6 * 256 queued
// SURF (tensor metrics with surface data or ridge storage): every length by
// len_tet_ani from the owner tet's xTetra edge tags and vertices.
template <bool ANI, bool TAGS, bool PAR, int W = 1, bool L = false, bool SURF = false>
__global__ __launch_bounds__(256, W) void k_prilen(StatArgs A, LenPart *parts) {
  __shared__ TetRec srec[2][256];
  __shared__ unsigned short q[LEN_QCAP + 2];     // + the spare entry of unset slots
  __shared__ unsigned wcnt[4];
  __shared__ long long kbase[2];                 // first tet of each LDS buffer
  __shared__ unsigned lcnt[10];
  LenAcc acc(lcnt);
  // The tets a workgroup takes, batch by batch (kb = first tet of a batch,
  // valid while kb <= k1): XCD-contiguous ranges, one per workgroup, in
  // increasing tet order (the ring's keys stay ordered); the shells and
  // points of the next z-layer of cells are another range's, read by the
  // same L2.
  const unsigned tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t lb = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t per = (A.ne + gridDim.x - 1) / gridDim.x;
  const int64_t k0 = 1 + lb * per;
  const int64_t k1 = min(A.ne, k0 + per - 1);
  unsigned head = 0, tail = 0;                   // ring positions (uniform)
  // each batch's records go to an LDS buffer; the next batch's are loaded at
  // the start of the batch and written to the other buffer after its rounds,
  // so the load is in flight during them (loaded from a clamped index: no
  // merge copy that would wait for it; records past k1 are never used)
  const int4 *recs = reinterpret_cast<const int4 *>(A.tets);
  {
    const int64_t kn = max<int64_t>(1, min(k0 + (int64_t)tid, A.ne));
    int4 *srow = reinterpret_cast<int4 *>(&srec[0][tid]);
    srow[0] = recs[2 * kn];
    srow[1] = recs[2 * kn + 1];
    // no second batch yet: a base no index reaches, in 64 and in 32 bits
    if (tid == 0) { kbase[0] = k0; kbase[1] = -(1LL << 40) + (1LL << 31); }
    __syncthreads();
  }

  int buf = 0;
  for (int64_t kb = k0;; buf ^= 1) {
    const bool more = kb <= k1;
    if (!more && head == tail) break;
    const unsigned prev_end = tail;              // entries before it: the previous batch
    const int64_t kbn = kb + 256;
    const int64_t kn = max<int64_t>(1, min(kbn + (int64_t)tid, A.ne));
    const int4 pv = recs[2 * kn], pn = recs[2 * kn + 1];
    if (more) {
      const int64_t k = kb + tid;
      const TetRec t = srec[buf][tid];
      unsigned m = 0;
      if (k <= k1) {
        const int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
        if (t.v[0] > 0 && !(TAGS && tet_4ridge(A, v))) {
          m = 0x3fu;
          if constexpr (!TAGS) {
            // a face neighbour with a smaller index disowns the face's three
            // edges (those not through the opposite local vertex f):
            // f = 0: edges 3,4,5; 1: 1,2,5; 2: 0,2,4; 3: 0,1,3 -- the same
            // test as "n0 or n1 smaller" per edge, n0/n1 = the neighbours
            // across the two faces that hold it
            const unsigned emask[4] = {0x38u, 0x26u, 0x15u, 0x0bu};
#pragma unroll
            for (int f = 0; f < 4; f++) {
              const int n = t.nb[f];
              bool sm;
              if constexpr (L) sm = (unsigned)n - 1u < (unsigned)k - 1u;   // 1 <= n < k
              else sm = n && n < k;
              m &= sm ? ~emask[f] : ~0u;
            }
          }
        }
      }
      // ring positions in (thread, ia) order: the wave's exclusive prefix of
      // the per-thread counts through one ballot per edge slot (mbcnt), the
      // wave totals in LDS
      unsigned pre = 0, wtot = 0;
#pragma unroll
      for (int ia = 0; ia < 6; ia++) {
        const unsigned long long bb = __ballot((m >> ia) & 1u);
        pre = __builtin_amdgcn_mbcnt_hi((unsigned)(bb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bb, pre));
        wtot += (unsigned)__popcll(bb);
      }
      if (lane == 0) wcnt[wv] = wtot;
      __syncthreads();
      unsigned base = 0, total = 0;
      for (unsigned w = 0; w < 4; w++) {
        base += (w < wv) ? wcnt[w] : 0u;
        total += wcnt[w];
      }
      total = __builtin_amdgcn_readfirstlane(total);
      unsigned pos = tail + base + pre;
      // unconditional stores: an unset slot writes the spare entry q[LEN_QCAP]
#pragma unroll
      for (int ia = 0; ia < 6; ia++) {
        const unsigned bit = (m >> ia) & 1u;
        q[bit ? (pos & (LEN_QCAP - 1)) : LEN_QCAP] = (unsigned short)((buf << 11) | (tid << 3) | ia);
        pos += bit;
      }
      __syncthreads();
      tail += total;
    }
    // full rounds; a partial one while entries of the previous batch remain
    // (their LDS records are rewritten next); everything once the tets ran out
    const unsigned avail = tail - head;
    unsigned nr = avail >> 8;
    if (!more) nr = (avail + 255u) >> 8;
    else if (head + (nr << 8) < prev_end) nr++;
    const long long kb0 = kbase[0], kb1 = kbase[1];   // fixed during the rounds
    for (unsigned r = 0; r < nr; r++) {
      const unsigned cnt = min(256u, tail - head);
      bool on = false;
      double len = 0.0;
      long long key = 0;
      if (tid < cnt) {
        const unsigned it = q[(head + tid) & (LEN_QCAP - 1)];
        const int eb = (int)(it >> 11), slot = (int)((it >> 3) & 255u), ia = (int)(it & 7u);
        // the record's fields by LDS address (no per-lane selects)
        const int *sv = srec[eb][slot].v, *sn = srec[eb][slot].nb;
        const int64_t kk = (eb ? kb1 : kb0) + slot;
        const int o0 = oth0(ia), o1 = oth1(ia);
        const int a = sv[iare0(ia)], b = sv[iare1(ia)], keep0 = sv[o1], keep1 = sv[o0];
        const int c0 = sn[o0], c1 = sn[o1];
        // the first rotation step's records, issued with the points' loads
        TetRec r0{}, r1{};
        // FLAT: the rotation's first two steps as straight-line selects (no
        // point tags)
        constexpr bool FLAT = !TAGS;
        if (c0) r0 = shell_rec<L>(A, srec, kb0, kb1, c0);
        if (c1) r1 = shell_rec<L>(A, srec, kb0, kb1, c1);
        FlatRot<L> fr{c0, c1, keep0, keep1, r0, r1};
        if constexpr (SURF) {
          const int vv[4] = {sv[0], sv[1], sv[2], sv[3]};
          len = len_tet_ani(A, vv, ia, a, b, A.etag ? (unsigned)A.etag[kk] : 0u);
        } else {
          len = edge_len_t<ANI>(A, a, b);
        }
        if constexpr (FLAT) {
          fr.step(A, srec, kb0, kb1, kk, a, b);
          fr.step(A, srec, kb0, kb1, kk, a, b);
          on = fr.finish(A, srec, kb0, kb1, kk, a, b) && !(PAR && par_excluded(A, a, b));
        } else
          on = owns_edge<TAGS, L>(A, srec, kb0, kb1, kk, a, b, c0, c1, keep0, keep1, r0, r1) &&
               !(PAR && par_excluded(A, a, b));
        if constexpr (L) key = LEN_STEP2 + (long long)(6u * (unsigned)kk + (unsigned)ia);   // 6 ne < 2^32
        else key = LEN_STEP2 + 6 * kk + ia;
      }
      if constexpr (L) acc.add_ordered(on, len, key);
      else acc.add(on, len, key);
      head += cnt;
    }
    if (more) {                                  // no entry of the previous batch is left
      __syncthreads();                           // ... once every wave is past its rounds
      int4 *srow = reinterpret_cast<int4 *>(&srec[buf ^ 1][tid]);
      srow[0] = pv;
      srow[1] = pn;
      if (tid == 0) kbase[buf ^ 1] = kbn;
    }
    __syncthreads();                             // srec, wcnt, kbase rewritten next
    kb = kbn;
  }
  acc.store(parts + lb);
}

// step 1 of the distributed prilen: the owned parallel edges, in list order,
// each once (src/quality_pmmg.c:445-502); one workgroup.  The kernel the
// reference selects at :462-466: MMG5_lenSurfEdg33_ani for a tensor metric in
// classic storage (isedg from the edge's hash tag), else MMG5_lenSurfEdg_iso
// -- for a tensor metric with metRidTyp = 1 on the flat array, as written
__global__ __launch_bounds__(256) void k_prilen_par(StatArgs A, const int2 *edges, const uint16_t *etags,
                                                    int64_t n, LenPart *part) {
  __shared__ unsigned lcnt[10];
  LenAcc acc(lcnt);
  for (int64_t base = 0; base < n; base += blockDim.x) {
    const int64_t i = base + threadIdx.x;
    const bool on = i < n;
    double len = 0.0;
    if (on) {
      const int2 e = edges[i];
      if (A.msize != 6) len = edge_len(A, e.x, e.y);
      else if (A.ridmet) len = len_iso_flat(A, e.x, e.y);
      else len = len_surf_ani(A, e.x, e.y, etags && (etags[i] & TAG_GEO), false);
    }
    acc.add(on, len, i);
  }
  acc.store(part);
}

// fixed-order reduction; the last level resolves the extremal edges' endpoints
// (step-1 keys: the list entry; step-2 keys: the tet's local edge)
__global__ __launch_bounds__(256) void k_prilen_final(const LenPart *parts, int n, LenPart *res,
                                                      pmx_len_part *pub, const TetRec *tets,
                                                      const int2 *par_edges) {
  __shared__ LenPart sh[256];
  LenPart p;
  len_init(p);
  const int pb = (n + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * pb, hi = min(n, lo + pb);
  int per = (hi - lo + 255) / 256;
  for (int b = lo + threadIdx.x * per; b < min(hi, lo + (int)(threadIdx.x + 1) * per); b++)
    len_merge(p, parts[b]);
  sh[threadIdx.x] = p;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) len_merge(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (res) res[blockIdx.x] = sh[0];
  if (pub) {
    const LenPart &r = sh[0];
    pmx_len_part o;
    o.avlen = r.avlen; o.lmin = r.ned ? r.lmin : 1.e30; o.lmax = r.lmax;
    o.ned = r.ned; o.nullEdge = r.nul;
    for (int i = 0; i < 9; i++) o.hl[i] = r.hl[i];
    o.amin = o.bmin = o.amax = o.bmax = 0;
    long long keys[2] = {r.kmin, r.kmax};
    long long ab[2][2] = {{0, 0}, {0, 0}};
    for (int j = 0; j < 2 && r.ned; j++) {
      const long long key = keys[j];
      if (key >= LEN_STEP2) {
        const long long kk = (key - LEN_STEP2) / 6;
        const int ia = (int)((key - LEN_STEP2) % 6);
        const TetRec t = tets[kk];
        ab[j][0] = pick_v(t, IARE[ia][0]);
        ab[j][1] = pick_v(t, IARE[ia][1]);
      } else {
        ab[j][0] = par_edges[key].x;
        ab[j][1] = par_edges[key].y;
      }
    }
    o.amin = ab[0][0]; o.bmin = ab[0][1]; o.amax = ab[1][0]; o.bmax = ab[1][1];
    *pub = o;
  }
}

// ---- host side ------------------------------------------------------------------

bool length_view(const pmx_call &C, int metRidTyp, StatArgs &A) {
  const pmx_ctx *ctx = C.ctx;
  A.ridmet = metRidTyp == 1 && A.msize == 6;
  if (A.ridmet && !A.ptag)
    return C.fail("metRidTyp = 1 with a tensor metric needs the point tags (pmx_upload_point_tags)");
  if (ctx->have_surf) {
    A.etag = ctx->d_etag.p;
    A.pn = ctx->d_pn.p;
    A.pxp = ctx->d_pxp.p;
    A.xpn = ctx->d_xpn.p;
  }
  return true;
}

extern "C" {

// Mmg's surface data of the background: packed on the host (the xTetra edge
// tags to 2 bits per edge of each tet, the normals and xPoint indices as
// arrays), checked, uploaded.  Replaces the previous upload's.
int pmx_upload_surface(pmx_ctx *ctx, const pmx_surface_view *sv) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_upload_surface", ctx->stream};
  ctx->have_surf = false;
  if (!ctx->have_bg) return C.fail("upload a background first");
  if (!sv) return 1;                        // no surface data: no xTetra, zero normals
  const int64_t np = ctx->np, ne = ctx->ne, nxt = sv->nxt, nxp = sv->nxp;
  if (nxt < 0 || nxp < 0 || (nxt > 0 && (!sv->tetra_xt || !sv->xtetra_tag || sv->tetra_stride < 4 ||
                                        sv->xtetra_stride < 12)) ||
      (!sv->point_n != !sv->point_xp) || (sv->point_n && sv->point_stride < 24) ||
      (nxp > 0 && (!sv->xpoint_n1 || !sv->xpoint_n2 || sv->xpoint_stride < 24)))
    return C.fail("bad view");
  hipSetDevice(ctx->device);
  std::vector<uint16_t> et((size_t)(ne + 1), 0);
  std::vector<double> pn((size_t)(np + 1) * 3, 0.0), xpn((size_t)(nxp + 1) * 6, 0.0);
  std::vector<int> pxp((size_t)(np + 1), 0);
  std::atomic<bool> bad{false};
  if (nxt > 0)
    pmx_par_for(1, ne + 1, [&](int64_t k0, int64_t k1) {
      for (int64_t k = k0; k < k1; k++) {
        const int xt = *(const int *)((const char *)sv->tetra_xt + k * sv->tetra_stride);
        if (xt == 0) continue;
        if (xt < 0 || xt > nxt) { bad = true; continue; }
        const uint16_t *tg = (const uint16_t *)((const char *)sv->xtetra_tag + (int64_t)xt * sv->xtetra_stride);
        unsigned b = 0;
        for (int ia = 0; ia < 6; ia++)
          b |= ((tg[ia] & PMX_TAG_BDY) ? 1u : 0u) << (2 * ia) | ((tg[ia] & PMX_TAG_GEO) ? 1u : 0u) << (2 * ia + 1);
        et[(size_t)k] = (uint16_t)b;
      }
    });
  if (sv->point_n)
    pmx_par_for(1, np + 1, [&](int64_t i0, int64_t i1) {
      for (int64_t i = i0; i < i1; i++) {
        const double *n = (const double *)((const char *)sv->point_n + i * sv->point_stride);
        const int xp = *(const int *)((const char *)sv->point_xp + i * sv->point_stride);
        if (xp < 0 || xp > nxp) { bad = true; continue; }
        pxp[(size_t)i] = xp;
        for (int c = 0; c < 3; c++) pn[(size_t)(3 * i + c)] = n[c];
      }
    });
  for (int64_t x = 1; x <= nxp; x++) {
    const double *n1 = (const double *)((const char *)sv->xpoint_n1 + x * sv->xpoint_stride);
    const double *n2 = (const double *)((const char *)sv->xpoint_n2 + x * sv->xpoint_stride);
    for (int c = 0; c < 3; c++) { xpn[(size_t)(6 * x + c)] = n1[c]; xpn[(size_t)(6 * x + 3 + c)] = n2[c]; }
  }
  if (bad) return C.fail("an xTetra or xPoint index is out of range");
  hipStream_t s = C.s;
  if (!pmx_dgrow(ctx, ctx->d_etag, et.size()) || !pmx_dgrow(ctx, ctx->d_pn, pn.size()) ||
      !pmx_dgrow(ctx, ctx->d_pxp, pxp.size()) || !pmx_dgrow(ctx, ctx->d_xpn, xpn.size()))
    return 0;
  PMX_CK(C, hipMemcpyAsync(ctx->d_etag.p, et.data(), et.size() * 2, hipMemcpyHostToDevice, s));
  PMX_CK(C, hipMemcpyAsync(ctx->d_pn.p, pn.data(), pn.size() * 8, hipMemcpyHostToDevice, s));
  PMX_CK(C, hipMemcpyAsync(ctx->d_pxp.p, pxp.data(), pxp.size() * 4, hipMemcpyHostToDevice, s));
  PMX_CK(C, hipMemcpyAsync(ctx->d_xpn.p, xpn.data(), xpn.size() * 8, hipMemcpyHostToDevice, s));
  PMX_CK(C, hipStreamSynchronize(s));
  ctx->have_surf = true;
  return 1;
}

int pmx_prilen_device(pmx_ctx *ctx, int metRidTyp, const pmx_par_edges *par, void *dev_result) {
  // metRidTyp (src/quality_pmmg.c:462,527): 0 or 1 give the same lengths for a
  // size-1 metric (MMG5_lenedg = lenedg_iso, MMG5_lenSurfEdg_iso); with a
  // size-6 metric 1 selects Mmg's ridge storage (length_view)
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_prilen", ctx->stream};
  if (!dev_result) return C.fail("dev_result is NULL");
  if (!check_met_rid_typ(C, metRidTyp)) return 0;
  hipSetDevice(ctx->device);
  StatArgs A;
  if (!stat_args(C, A)) return 0;
  if (ctx->sd.imet < 0) return C.fail("no metric");
  if (ctx->ne >= (1LL << 29)) return C.fail("ne >= 2^29 per group");
  if (!length_view(C, metRidTyp, A)) return 0;
  const bool ani = A.msize == 6;
  hipStream_t s = C.s;
  // parallel edges (host): step-1 list (owned, first occurrence, list order)
  // and the sorted keys of the edges step 2 must not count
  std::vector<int2> own;
  std::vector<uint16_t> own_tag;
  std::vector<unsigned long long> excl;
  std::vector<uint8_t> ppt;
  if (par && par->n > 0) {
    if (!par->a || !par->b || !par->owner) return C.fail("bad parallel edges");
    std::unordered_set<unsigned long long> popped;
    for (int64_t i = 0; i < par->n; i++) {
      const int a = par->a[i], b = par->b[i];
      if (a < 1 || b < 1 || a > ctx->np || b > ctx->np || a == b)
        return C.fail("parallel edge vertex out of range");
      const unsigned long long key = ((unsigned long long)(unsigned)std::min(a, b) << 32) | (unsigned)std::max(a, b);
      if (par->owner[i] == par->myrank) {
        // MMG5_hashPop succeeds once per edge: a repeated entry is not counted
        if (popped.insert(key).second) {
          own.push_back(make_int2(a, b));
          own_tag.push_back(par->tag ? par->tag[i] : (uint16_t)0);
        }
        excl.push_back(key);
      } else if (par->exact_once) {
        excl.push_back(key);
      }
    }
    std::sort(excl.begin(), excl.end());
    excl.erase(std::unique(excl.begin(), excl.end()), excl.end());
    ppt.assign((size_t)(ctx->np + 1), 0);
    for (unsigned long long key : excl) {
      ppt[(size_t)(key >> 32)] = 1;
      ppt[(size_t)(key & 0xffffffffu)] = 1;
    }
  }
  using KFn = void (*)(StatArgs, LenPart *);
  // variants: metric kind x point tags x parallel edges (each drops the
  // other paths' registers and branches)
  // the isotropic variants held to 5 waves per SIMD (96 VGPRs, a few
  // spills): 2 % faster at the C5 share; the anisotropic ones spill too
  // much there (4.46 instead of 3.63 ms) and keep the compiler's choice
  static const KFn kfn[16] = {
      k_prilen<false, false, false, 5>,        k_prilen<false, false, true, 5>,
      k_prilen<false, true, false, 5>,         k_prilen<false, true, true, 5>,
      k_prilen<true, false, false>,            k_prilen<true, false, true>,
      k_prilen<true, true, false>,             k_prilen<true, true, true>,
      k_prilen<false, false, false, 5, true>,  k_prilen<false, false, true, 5, true>,
      k_prilen<false, true, false, 5, true>,   k_prilen<false, true, true, 5, true>,
      k_prilen<true, false, false, 1, true>,   k_prilen<true, false, true, 1, true>,
      k_prilen<true, true, false, 1, true>,    k_prilen<true, true, true, 1, true>};
  // lean 32-bit index arithmetic while 6 ne + 5 fits 32 bits (PMX_PRILEN_WIDE=1:
  // the 64-bit variant whatever the size)
  static const bool wide = getenv("PMX_PRILEN_WIDE") != nullptr;
  const bool lean = !wide && A.ne < 700000000LL;
  const int sel = (lean ? 8 : 0) | (ani ? 4 : 0) | (A.ptag ? 2 : 0) |
                  (par && par->n > 0 && !excl.empty() ? 1 : 0);
  // tensor metrics measured along the surface / in ridge storage
  // (len_tet_ani): the owner tet's xTetra tags and vertices per edge
  // (held to 4 waves per SIMD: they sit at the 128-VGPR edge, where the
  // compiler's own choice falls on either side of it)
  static const KFn kfs[8] = {
      k_prilen<true, false, false, 4, false, true>, k_prilen<true, false, true, 4, false, true>,
      k_prilen<true, true, false, 4, false, true>,  k_prilen<true, true, true, 4, false, true>,
      k_prilen<true, false, false, 4, true, true>,  k_prilen<true, false, true, 4, true, true>,
      k_prilen<true, true, false, 4, true, true>,   k_prilen<true, true, true, 4, true, true>};
  const bool surf = ani && (ctx->have_surf || A.ridmet);
  const KFn kern = surf ? kfs[(lean ? 4 : 0) | (sel & 3)] : kfn[sel];
  const int nb = stat_blocks(ctx->ne);
  if (!ensure_red(ctx, sizeof(LenPart) * ((size_t)nb + 1 + FINAL_GRID + 1))) return 0;
  LenPart *parts = (LenPart *)ctx->d_red.p;
  A.npar = (int64_t)excl.size();
  if (A.npar) {
    if (!pmx_dgrow(ctx, ctx->d_pkey, excl.size()) || !pmx_dgrow(ctx, ctx->d_ppt, ppt.size()) ||
        !pmx_dgrow(ctx, ctx->d_pedge, std::max<size_t>(own.size(), 1)) ||
        !pmx_dgrow(ctx, ctx->d_pedge_tag, std::max<size_t>(own.size(), 1)))
      return 0;
    PMX_CK(C, hipMemcpyAsync(ctx->d_pkey.p, excl.data(), excl.size() * 8, hipMemcpyHostToDevice, s));
    PMX_CK(C, hipMemcpyAsync(ctx->d_ppt.p, ppt.data(), ppt.size(), hipMemcpyHostToDevice, s));
    if (!own.empty()) {
      PMX_CK(C, hipMemcpyAsync(ctx->d_pedge.p, own.data(), own.size() * sizeof(int2), hipMemcpyHostToDevice, s));
      PMX_CK(C, hipMemcpyAsync(ctx->d_pedge_tag.p, own_tag.data(), own_tag.size() * sizeof(uint16_t),
                               hipMemcpyHostToDevice, s));
    }
    A.par_key = ctx->d_pkey.p;
    A.par_pt = ctx->d_ppt.p;
  }
  // partials: [0] step 1 (owned parallel edges), [1..nb] step 2 (tet edges)
  if (!own.empty())
    hipLaunchKernelGGL(k_prilen_par, dim3(1), dim3(256), 0, s, A, ctx->d_pedge.p,
                       (const uint16_t *)ctx->d_pedge_tag.p, (int64_t)own.size(), parts);
  else
    hipLaunchKernelGGL(k_prilen_par, dim3(1), dim3(256), 0, s, A, (const int2 *)nullptr, (const uint16_t *)nullptr,
                       (int64_t)0, parts);
  hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, A, parts + 1);
  LenPart *mid = parts + 1 + nb;
  hipLaunchKernelGGL(k_prilen_final, dim3(FINAL_GRID), dim3(256), 0, s, parts, nb + 1, mid,
                     (pmx_len_part *)nullptr, ctx->d_tets.p, (const int2 *)ctx->d_pedge.p);
  hipLaunchKernelGGL(k_prilen_final, dim3(1), dim3(256), 0, s, mid, FINAL_GRID, (LenPart *)nullptr,
                     (pmx_len_part *)dev_result, ctx->d_tets.p, (const int2 *)ctx->d_pedge.p);
  PMX_CK(C, hipGetLastError());
  return 1;
}

int pmx_prilen(pmx_ctx *ctx, int metRidTyp, const pmx_par_edges *par, pmx_len_stats *st) {
  if (!ctx) return 0;
  const pmx_call C{ctx, "pmx_prilen", ctx->stream};
  if (!st) return C.fail("st is NULL");
  hipSetDevice(ctx->device);
  if (!pmx_dgrow(ctx, ctx->d_pub, 32)) return 0;
  if (!pmx_prilen_device(ctx, metRidTyp, par, ctx->d_pub.p)) return 0;
  pmx_len_part r;
  if (!read_pub(C, r)) return 0;
  len_to_stats(r, st);
  return 1;
}

}  // extern "C"
