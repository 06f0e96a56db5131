// pmx_walk.hip -- the volume kernels: k_walks (production) and k_walk
// (reference-order walk, kept for the parity tests), locate + interpolate.
//
// One thread per new volume vertex, adjacency walk from the hint grid
// (PMMG_locatePointVol, reference src/locate_pmmg.c:786-883), fused
// PMMG_interp4bar_{iso,ani} (src/interpmesh_pmmg.c:206-270), stuck lanes and
// near-face ties compacted into lists for k_fallback.  What makes a step cheap:
//
//  * direction without divisions: a walk step only needs the ORDER of the
//    barycentrics and the sign test lambda_min > -1e-6.  The exact quotients
//    lambda_f = -num_f/vol (src/barycoord_pmmg.c:238-257) are formed only once
//    the estimate comes within a guard of the threshold; "found" and the
//    barycentrics used for the interpolation are exactly the reference's.  The
//    answer does not depend on the path (unique containing tet, or the
//    canonical min-index tet of a tie -- canonical_tet).
//  * vertex reuse: the next tet shares a face (3 vertices) with the current
//    one; only its opposite vertex is gathered.
//  * layout specialisation: the interpolation is compiled for the solution
//    layout (one anisotropic metric; S isotropic/vector components; generic)
//    so the register allocation is not the maximum over every layout.
#include <algorithm>
#include "pmx_device.h"
#include "pmx_kernels.h"

#define WALK_RING 4
#define TIE_NEAR 1.e-5
#define APPROX_GUARD 1.e-13

__device__ __forceinline__ int64_t walk_xcd_remap(int64_t b, int64_t nb) {
  // blocks b and b+8 share an XCD (round-robin dispatch): each XCD gets a
  // contiguous range of the Morton-ordered queries so its L2 sees neighbours
  int64_t xcd = b & 7, r = b >> 3, q = nb >> 3, rem = nb & 7;
  return (xcd < rem) ? xcd * (q + 1) + r : rem * (q + 1) + (xcd - rem) * q + r;
}

__device__ __forceinline__ int wclamp(double t, int n) {
  if (!(t > 0.0)) return 0;                 // also catches NaN
  if (t >= (double)(n - 1)) return n - 1;
  return (int)t;
}

// empty hint cell: nearest non-empty cell in growing shells (rare; kept out of
// line so that its loops do not inflate the walk's register allocation)
// (the grid's dims as scalars: a GridDesc argument of this out-of-line call
// would be passed through scratch, 16 -> 112 B per lane in k_walks)
__device__ __noinline__ int hint_search(const int *grid, int gx, int gy, int gz, int cx, int cy,
                                        int cz) {
  for (int r = 1; r <= 3; r++) {
    for (int dz = -r; dz <= r; dz++)
      for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++) {
          if (max(abs(dx), max(abs(dy), abs(dz))) != r) continue;
          int x = cx + dx, y = cy + dy, z = cz + dz;
          if (x < 0 || y < 0 || z < 0 || x >= gx || y >= gy || z >= gz) continue;
          int kk = grid[(int64_t)x + (int64_t)gx * ((int64_t)y + (int64_t)gy * z)];
          if (kk) return kk;
        }
  }
  return 1;
}

__device__ __forceinline__ int walk_hint(const int *grid, const GridDesc &g, D3 p) {
  int cx = wclamp((p.x - g.lo[0]) * g.inv[0], g.dim[0]);
  int cy = wclamp((p.y - g.lo[1]) * g.inv[1], g.dim[1]);
  int cz = wclamp((p.z - g.lo[2]) * g.inv[2], g.dim[2]);
  int k = grid[gcell(g, cx, cy, cz)];
  return k ? k : hint_search(grid, g.dim[0], g.dim[1], g.dim[2], cx, cy, cz);
}

// numerators of the barycentrics: lambda_f = -num_f / vol, with exactly the
// operations of tet_lambda (pmx_device.h) before its division
__device__ __forceinline__ void face_nums(const D3 P[4], D3 p, double num[4], double *volp) {
  double vol = orvol(P[0], P[1], P[2], P[3]);
  D3 n0 = nonunit_normal(P[1], P[2], P[3]);
  D3 n1 = nonunit_normal(P[0], P[3], P[2]);
  D3 n2 = nonunit_normal(P[0], P[1], P[3]);
  D3 n3 = nonunit_normal(P[0], P[2], P[1]);
  num[0] = (p.x - P[1].x) * n0.x + (p.y - P[1].y) * n0.y + (p.z - P[1].z) * n0.z;
  num[1] = (p.x - P[0].x) * n1.x + (p.y - P[0].y) * n1.y + (p.z - P[0].z) * n1.z;
  num[2] = (p.x - P[0].x) * n2.x + (p.y - P[0].y) * n2.y + (p.z - P[0].z) * n2.z;
  num[3] = (p.x - P[0].x) * n3.x + (p.y - P[0].y) * n3.y + (p.z - P[0].z) * n3.z;
  *volp = vol;
}

__device__ __forceinline__ void wranks(const double l[4], int rk[4]) {
  rk[0] = rk[1] = rk[2] = rk[3] = 0;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = a + 1; b < 4; b++) {
      bool bfirst = l[b] < l[a];          // stable: b after a unless strictly smaller
      rk[a] += bfirst ? 1 : 0;
      rk[b] += bfirst ? 0 : 1;
    }
}

__device__ __forceinline__ void wave_stats_w(uint4 *rec, unsigned cnt, unsigned sum, unsigned mx,
                                             unsigned mn) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sum += __shfl_xor(sum, o, 64);
    unsigned a = __shfl_xor(mx, o, 64), b = __shfl_xor(mn, o, 64);
    mx = a > mx ? a : mx;
    mn = b < mn ? b : mn;
  }
  if ((threadIdx.x & 63) == 0) *rec = make_uint4(cnt, sum, mx, mn);
}

// a[i] for a 4-array held in registers: masked OR (a select chain is turned
// back into an indexed private-array load, i.e. scratch, by the compiler)
__device__ __forceinline__ int pick4(const int a[4], int i) {
  return (a[0] & -(int)(i == 0)) | (a[1] & -(int)(i == 1)) | (a[2] & -(int)(i == 2)) |
         (a[3] & -(int)(i == 3));
}

__device__ __forceinline__ D3 dsel(bool c, D3 a, D3 b) {
  return D3{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z};
}

// ---- layout-specialised interpolation: interp_layout (pmx_device.h) ---------

// layout of the solutions for the walk kernel
static int walk_layout(const SolDesc &sd, int *S) {
  *S = sd.S;
  if (sd.nsol == 1 && sd.size[0] == 6 && sd.imet == 0 && !sd.metric_const) return LAYOUT_ANI;
  bool iso = !sd.metric_const && sd.S >= 1 && sd.S <= 8;
  for (int s = 0; s < sd.nsol; s++) iso = iso && sd.size[s] != 6;
  return iso ? LAYOUT_ISO : LAYOUT_GEN;
}

// Near-face cases of the canonical tie rule resolved in place (canonical_tet,
// pmx_fallback.hip, is the general BFS over the containing set; this is the
// same rule for the two shapes that make up almost every tie):
//  * no near face has an interior neighbour: the set is {cur};
//  * exactly one near face f with neighbour n: the set is {cur} if n does not
//    contain p, {cur, n} if it does and n has no further near face with an
//    interior neighbour other than cur -> min(cur, n).
// Returns true when the general BFS is needed (edge / vertex ties, chains).
// On return false, cur/t/lam hold the canonical tet and its barycentrics.
__device__ __forceinline__ bool face_tie(const VolArgs &A, D3 p, int &cur, TetRec &t, double lam[4]) {
  int nnear = 0, f1 = 0;
#pragma unroll
  for (int f = 0; f < 4; f++) {
    const bool nf = t.nb[f] != 0 && lam[f] < TIE_NEAR;
    nnear += nf ? 1 : 0;
    f1 = nf ? f : f1;
  }
  if (nnear == 0) return false;
  if (nnear > 1) return true;
  const int n = wrec_resolve(pick4(t.nb, f1), A.tets, cur);   // a far field of a compact record
  const TetRec u = A.tets[n];
  if (u.v[0] <= 0) return false;
  const D3 Q[4] = {ld3(A.xyz, u.v[0]), ld3(A.xyz, u.v[1]), ld3(A.xyz, u.v[2]), ld3(A.xyz, u.v[3])};
  double mu[4], vu;
  tet_lambda(Q, p, mu, &vu);
  if (!(fmin(fmin(mu[0], mu[1]), fmin(mu[2], mu[3])) > -PMX_EPS)) return false;
  bool more = false;
#pragma unroll
  for (int g = 0; g < 4; g++) more |= (u.nb[g] != 0 && u.nb[g] != cur && mu[g] < TIE_NEAR);
  if (more) return true;
  if (n < cur) {
    cur = n;
    t = u;
#pragma unroll
    for (int f = 0; f < 4; f++) lam[f] = mu[f];
  }
  return false;
}

// the end of a lane: interpolate, or hand the point to k_fallback (k_walk, and
// k_walks for the generic layout; walk_finish_wave below for the others)
template <int LAYOUT, int S, bool TIES>
__device__ __forceinline__ void walk_finish(const VolArgs &A, int64_t i, D3 p, bool found, int step,
                                            int cur, TetRec &t, double lam[4], unsigned &s_cnt,
                                            unsigned &s_sum, unsigned &s_max, unsigned &s_min) {
  if (found) {
    double lmn = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
    if (lmn < TIE_NEAR && (!TIES || face_tie(A, p, cur, t, lam))) {
      // within the tolerance of several tets: canonical tet by the BFS
      unsigned slot = atomicAdd(A.tie_count, 1u);
      A.tie_list[slot] = make_int2((int)i, cur);
      A.steps[i] = step;
      return;
    }
    A.elem[i] = cur;
    const int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
    A.status[i] = 1;
    A.steps[i] = step;
    unsigned wm = interp_layout<LAYOUT, S>(A.sol, A.sd, v, lam, A.out + i * A.sd.S);
    A.wmask[i] = (uint8_t)(wm | A.const_bit);
    s_cnt += 1; s_sum += step;
    s_max = max(s_max, (unsigned)step); s_min = min(s_min, (unsigned)step);
  } else {
    unsigned slot = atomicAdd(A.stuck_count, 1u);
    A.stuck_list[slot] = (int)i;
    A.found[slot] = 0x7fffffff;
    A.bestk[slot] = 0x7fffffff;
    A.best[slot] = ~0ull;
    A.steps[i] = -step;
  }
}

// The end of a wave of k_walks (LAYOUT_ANI / LAYOUT_ISO): walk_finish's results,
// with the rows of a wave whose 64 points are consecutive stored as one block.
//
// Every lane of the wave comes here, also one past the list's end: it has
// walked no step (every listed point counts one step or more).
// A lane has a row when its point is found, stays out of the tie and stuck
// lists and its interpolation wrote something.  A lane's own stores scatter
// 8-16-B pieces at a stride of 8 S bytes: three instructions over the 40
// 64-B segments of a wave's rows at S = 5.  When every lane has a row and
// lane l holds point i0 + l (the classification's compaction keeps the input
// order, so that is the normal case), the rows are 64 S consecutive doubles:
// they pass through the wave's own LDS slice and leave as S stores of 512
// consecutive bytes, 8-9 segments each.  Any other wave (a hole in its list
// window, a tie or stuck lane, a failed inversion, the tail) stores per lane,
// as walk_finish does.  The same doubles reach the same addresses either way.
// A located lane loads its solution rows before it stores anything: loads and
// stores share one in-order counter, so a store issued first would make the
// first use of a row wait for its acknowledgement as well.
template <int LAYOUT, int S, bool TIES>
__device__ __forceinline__ void walk_finish_wave(const VolArgs &A, int64_t i, D3 p, bool found,
                                                 int step, int cur, TetRec &t, double lam[4],
                                                 unsigned &s_cnt, unsigned &s_sum, unsigned &s_max,
                                                 unsigned &s_min) {
  __shared__ double rows[4][64 * S];               // a slice per wave of the 256-thread block
  bool located = false;
  if (step != 0) {
    if (found) {
      double lmn = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
      if (lmn < TIE_NEAR && (!TIES || face_tie(A, p, cur, t, lam))) {
        // within the tolerance of several tets: canonical tet by the BFS
        unsigned slot = atomicAdd(A.tie_count, 1u);
        A.tie_list[slot] = make_int2((int)i, cur);
        A.steps[i] = step;
      } else {
        located = true;
      }
    } else {
      unsigned slot = atomicAdd(A.stuck_count, 1u);
      A.stuck_list[slot] = (int)i;
      A.found[slot] = 0x7fffffff;
      A.bestk[slot] = 0x7fffffff;
      A.best[slot] = ~0ull;
      A.steps[i] = -step;
    }
  }
  double r[S];
  bool row = false;
  if (located) {
    const int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
    row = interp_row<LAYOUT, S>(A.sol, v, lam, r);
  }
  const int lane = threadIdx.x & 63;
  const int i0 = __builtin_amdgcn_readfirstlane((int)i);
  if (__all(row && (int)i == i0 + lane)) {
    double *w = rows[threadIdx.x >> 6];
#pragma unroll
    for (int k = 0; k < S; k++) w[lane * S + k] = r[k];
    // the wave reads what its other lanes wrote: LDS serves a wave's accesses
    // in order; the fences and the barrier keep the compiler to that order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double *o = A.out + (int64_t)i0 * S;
#pragma unroll
    for (int k = 0; k < S; k++) o[64 * k + lane] = w[64 * k + lane];
  } else if (row) {
    store_row<S>(r, A.out + i * S);
  }
  if (located) {
    A.elem[i] = cur;
    A.status[i] = 1;
    A.steps[i] = step;
    const unsigned wm = !row ? 0u : LAYOUT == LAYOUT_ANI ? 1u : (1u << A.sd.nsol) - 1u;
    A.wmask[i] = (uint8_t)(wm | A.const_bit);
    s_cnt += 1; s_sum += step;
    s_max = max(s_max, (unsigned)step); s_min = min(s_min, (unsigned)step);
  }
}

// ---- k_walk: the reference's walk order ----------------------------------------
// PM (PMX_RUN_POINTMAP): the start tet is the one resolved from the point's
// source vertex (A.grid then holds one start per list entry) instead of the
// hint grid's
template <int LAYOUT, int S, bool TIES, bool PM = false>
__global__ __launch_bounds__(256) void k_walk(VolArgs A) {
  const int64_t b = walk_xcd_remap(blockIdx.x, gridDim.x);
  const int64_t j = b * blockDim.x + threadIdx.x;
  unsigned s_cnt = 0, s_sum = 0, s_max = 0, s_min = 0xffffffffu;

  if (j < *A.nlist_dev) {     // the step's count (the grid is sized by an upper bound)
    const int64_t i = A.list[j];
    const D3 p{A.q[3 * i], A.q[3 * i + 1], A.q[3 * i + 2]};
    int cur;
    if constexpr (PM) cur = A.grid[j];
    else cur = walk_hint(A.grid, A.g, p);
    if (A.rec_start) A.start[i] = cur;
    int ring[WALK_RING];
#pragma unroll
    for (int r = 0; r < WALK_RING; r++) ring[r] = 0;
    int step = 0;
    bool found = false;
    TetRec t = A.tets[cur];
    D3 P[4];
    double lam[4];
    if (t.v[0] <= 0) step = 1;                        // !MG_EOK start: let the scan decide
    else {
      P[0] = ld3(A.xyz, t.v[0]); P[1] = ld3(A.xyz, t.v[1]);
      P[2] = ld3(A.xyz, t.v[2]); P[3] = ld3(A.xyz, t.v[3]);
      for (;;) {
        step++;
        double num[4], vol;
        face_nums(P, p, num, &vol);
        const double rv = 1.0 / vol;
#pragma unroll
        for (int f = 0; f < 4; f++) lam[f] = -(num[f] * rv);
        double lmin = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
        if (lmin > -PMX_EPS - APPROX_GUARD) {
          // near or inside: the reference's quotients decide
#pragma unroll
          for (int f = 0; f < 4; f++) lam[f] = -num[f] / vol;
          lmin = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
          if (lmin > -PMX_EPS) { found = true; break; }     // src/barycoord_pmmg.c:102-107
        }
        if (step >= A.max_walk) break;
        int rk[4];
        wranks(lam, rk);
#pragma unroll
        for (int r = WALK_RING - 1; r > 0; r--) ring[r] = ring[r - 1];
        ring[0] = cur;
        // first interior, not recently visited neighbour in ascending-lambda
        // order (src/locate_pmmg.c:819-833)
        int next = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          int f = (rk[0] == r) ? 0 : (rk[1] == r) ? 1 : (rk[2] == r) ? 2 : 3;
          int nb = pick4(t.nb, f);
          bool seen = false;
#pragma unroll
          for (int q = 0; q < WALK_RING; q++) seen |= (ring[q] == nb);
          if (!next && nb && !seen) next = nb;
        }
        if (!next) break;
        const TetRec u = A.tets[next];
        cur = next;
        if (u.v[0] <= 0) { t = u; break; }                  // !MG_EOK: let the scan decide
        // shared face: permute the known coordinates, gather the new vertex
        bool m[4][4];
        int nnew = 0, lnew = 0;
#pragma unroll
        for (int l = 0; l < 4; l++) {
#pragma unroll
          for (int k = 0; k < 4; k++) m[l][k] = (u.v[l] == t.v[k]);
          bool any = m[l][0] | m[l][1] | m[l][2] | m[l][3];
          nnew += any ? 0 : 1;
          lnew = any ? lnew : l;
        }
        if (nnew == 1) {
          const D3 pn = ld3(A.xyz, pick4(u.v, lnew));
          D3 Q[4];
#pragma unroll
          for (int l = 0; l < 4; l++)
            Q[l] = dsel(m[l][0], P[0], dsel(m[l][1], P[1], dsel(m[l][2], P[2], dsel(m[l][3], P[3], pn))));
#pragma unroll
          for (int l = 0; l < 4; l++) P[l] = Q[l];
        } else {                                               // inconsistent adjacency
          P[0] = ld3(A.xyz, u.v[0]); P[1] = ld3(A.xyz, u.v[1]);
          P[2] = ld3(A.xyz, u.v[2]); P[3] = ld3(A.xyz, u.v[3]);
        }
        t = u;
      }
    }
    walk_finish<LAYOUT, S, TIES>(A, i, p, found, step, cur, t, lam, s_cnt, s_sum, s_max, s_min);
  }
  wave_stats_w(A.wstats + (b * blockDim.x + threadIdx.x) / 64, s_cnt, s_sum, s_max, s_min);
}

// ---- k_walks: the slot walk (production) -------------------------------------
//
// The walk DIRECTION needs neither the reference's operation order nor the
// tet's own vertex order -- only "found" and the interpolation weights must be
// the reference's quotients.  k_walks therefore walks on slot-ordered state:
//  * slot k holds a vertex id I[k], its coordinates C[k] and the neighbour
//    NB[k] across the face opposite it; a step through the face opposite slot
//    s replaces slot s by the neighbour's fourth vertex (one select per slot,
//    instead of permuting all four coordinates into the new tet's order);
//  * the barycentric numerators are signed sub-volumes about p: with
//    d_k = C_k - p, w0 = d1.(d2 x d3), w1 = -d0.(d2 x d3), w2 = d3.(d0 x d1),
//    w3 = -d2.(d0 x d1) and vol = sum w (2 cross + 4 dot products, no
//    division); every step reflects the slot order's orientation, so the
//    sign flips;
//  * the lane leaves the loop when min w > -(EPS + SLOT_GUARD) vol (the
//    reference's threshold with a margin far above this estimate's error);
//    then, once per lane, the coordinates are put in tet order and the
//    reference's quotients (tet_lambda's operations) decide.  A candidate
//    they reject continues with the reference-order walk of k_walk.
// The located tet does not depend on the path (unique containing tet, or the
// canonical tet of a tie), so k_walks returns k_walk's results bit for bit.
#define SLOT_GUARD 1.e-10

__device__ __forceinline__ D3 dcross(D3 a, D3 b) {
  return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// one reference-order step decision (k_walk's): the first interior, not
// recently visited neighbour in ascending-lambda order; 0 if none
__device__ __forceinline__ int exact_next(const TetRec &t, const double lam[4], int ring[WALK_RING],
                                          int cur) {
  int rk[4];
  wranks(lam, rk);
#pragma unroll
  for (int r = WALK_RING - 1; r > 0; r--) ring[r] = ring[r - 1];
  ring[0] = cur;
  int next = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    int f = (rk[0] == r) ? 0 : (rk[1] == r) ? 1 : (rk[2] == r) ? 2 : 3;
    int nb = pick4(t.nb, f);
    bool seen = false;
#pragma unroll
    for (int q = 0; q < WALK_RING; q++) seen |= (ring[q] == nb);
    if (!next && nb && !seen) next = nb;
  }
  return next;
}

// the walk's tet record: through the compact copy (CW) or the full record
// (whole: run-flag experiment 17 -- a record with a far field is read whole
// from the 32-B records instead of resolving the chosen field)
template <bool CW>
__device__ __forceinline__ TetRec walk_rec(const VolArgs &A, int k, bool whole = false) {
  if constexpr (CW) {
    TetRec t = wrec_load(A.wrec, A.tets, k);
    if (whole && (t.nb[0] | t.nb[1] | t.nb[2] | t.nb[3]) < 0) t = A.tets[k];
    return t;
  } else {
    return A.tets[k];
  }
}

// FAR: the compact records have far neighbour fields (VolArgs.far); without
// them the walk compiles no resolution path
// PM: as in k_walk
template <int LAYOUT, int S, bool TIES, bool CW, bool FAR = true, bool PM = false>
__global__ __launch_bounds__(256) void k_walks(VolArgs A) {
  const int64_t b = walk_xcd_remap(blockIdx.x, gridDim.x);
  const int64_t j = b * blockDim.x + threadIdx.x;
  unsigned s_cnt = 0, s_sum = 0, s_max = 0, s_min = 0xffffffffu;
  // a lane's state at the end of its walk, for the wave's common epilogue
  // (step stays 0 in a lane past the list's end, and only there)
  int64_t i = 0;
  D3 p{0.0, 0.0, 0.0};
  TetRec t;
  int cur = 0, step = 0;
  bool found = false;
  double lam[4];

  if (j < *A.nlist_dev) {     // the step's count (the grid is sized by an upper bound)
    // the list keeps the input order (order-preserving compaction): the
    // point reads through it are as coalesced as the list itself (r03: a
    // list-ordered copy of the coordinates saved the walk 1 % and cost the
    // classification 0.15 ms of copying)
    i = A.list[j];
    p = D3{A.q[3 * i], A.q[3 * i + 1], A.q[3 * i + 2]};
    if constexpr (PM) {
      cur = A.grid[j];
      t = walk_rec<CW>(A, cur, FAR && A.exp == 17);
    } else {
      cur = walk_hint(A.grid, A.g, p);
      t = walk_rec<CW>(A, cur, FAR && A.exp == 17);
    }
    if (A.rec_start) A.start[i] = cur;
    int ring[WALK_RING];
#pragma unroll
    for (int r = 0; r < WALK_RING; r++) ring[r] = 0;
    if (t.v[0] <= 0) step = 1;                  // !MG_EOK start: let the scan decide
    else {
      D3 C[4] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2]), ld3(A.xyz, t.v[3])};
      int I[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
      int NB[4] = {t.nb[0], t.nb[1], t.nb[2], t.nb[3]};
      bool neg = false, cand = false;
      for (;;) {
        step++;
        D3 d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = D3{C[k].x - p.x, C[k].y - p.y, C[k].z - p.z};
        const D3 c23 = dcross(d[2], d[3]), c01 = dcross(d[0], d[1]);
        double w[4] = {ddot(d[1], c23), -ddot(d[0], c23), ddot(d[3], c01), -ddot(d[2], c01)};
        if (neg) {
#pragma unroll
          for (int k = 0; k < 4; k++) w[k] = -w[k];
        }
        const double vol = (w[0] + w[1]) + (w[2] + w[3]);
        const double wmin = fmin(fmin(w[0], w[1]), fmin(w[2], w[3]));
        // near or inside (or a degenerate / inverted tet): the reference decides
        if (!(vol > 0.0) || wmin > -(PMX_EPS + SLOT_GUARD) * vol) { cand = true; break; }
        if (step >= A.max_walk) break;
#pragma unroll
        for (int r = WALK_RING - 1; r > 0; r--) ring[r] = ring[r - 1];
        ring[0] = cur;
        // the admissible slot (interior, not recently visited neighbour) with
        // the smallest barycentric
        // smallest barycentric; a far field (< 0, pmx_wrec.h) counts as
        // admissible until it is chosen, then is resolved from the full record
        // and the choice made again (the same choice as on resolved fields)
        auto choose = [&]() {
          int sb = -1;
          double wb = 0.0;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int nb = NB[k];
            bool seen = false;
#pragma unroll
            for (int q = 0; q < WALK_RING; q++) seen |= (ring[q] == nb);
            const bool take = nb && !seen && (sb < 0 || w[k] < wb);
            sb = take ? k : sb;
            wb = take ? w[k] : wb;
          }
          return sb;
        };
        int sb = choose();
        if (FAR && sb >= 0 && pick4(NB, sb) < 0) {         // rare: a far field chosen
          for (int it = 0; it < 4 && sb >= 0 && pick4(NB, sb) < 0; it++) {
            const int r = wrec_resolve(pick4(NB, sb), A.tets, cur);
#pragma unroll
            for (int k = 0; k < 4; k++) NB[k] = (k == sb) ? r : NB[k];
            sb = choose();
          }
        }
        if (sb < 0) break;
        const int next = pick4(NB, sb);
        const TetRec u = walk_rec<CW>(A, next, FAR && A.exp == 17);
        cur = next;
        t = u;
        if (u.v[0] <= 0) break;                            // !MG_EOK: let the scan decide
        // the neighbour's fourth vertex replaces slot sb
        int nnew = 0, lnew = 0;
#pragma unroll
        for (int l = 0; l < 4; l++) {
          const bool any = (u.v[l] == I[0]) | (u.v[l] == I[1]) | (u.v[l] == I[2]) | (u.v[l] == I[3]);
          nnew += any ? 0 : 1;
          lnew = any ? lnew : l;
        }
        if (nnew != 1) {                                   // inconsistent adjacency: reload
#pragma unroll
          for (int k = 0; k < 4; k++) {
            C[k] = ld3(A.xyz, u.v[k]);
            I[k] = u.v[k];
            NB[k] = u.nb[k];
          }
          neg = false;
          continue;
        }
        const int vn = pick4(u.v, lnew);
        const D3 pn = ld3(A.xyz, vn);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          C[k] = dsel(k == sb, pn, C[k]);
          I[k] = (k == sb) ? vn : I[k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
          NB[k] = (u.nb[0] & -(int)(u.v[0] == I[k])) | (u.nb[1] & -(int)(u.v[1] == I[k])) |
                  (u.nb[2] & -(int)(u.v[2] == I[k])) | (u.nb[3] & -(int)(u.v[3] == I[k]));
        neg = !neg;
      }
      if (cand) {
        // coordinates in tet order, then the reference's quotients; a
        // rejected candidate continues in the reference's order (rare)
        D3 P[4];
#pragma unroll
        for (int l = 0; l < 4; l++)
          P[l] = dsel(t.v[l] == I[0], C[0],
                      dsel(t.v[l] == I[1], C[1], dsel(t.v[l] == I[2], C[2], C[3])));
        for (;;) {
          double num[4], vol;
          face_nums(P, p, num, &vol);
#pragma unroll
          for (int f = 0; f < 4; f++) lam[f] = -num[f] / vol;
          const double lmin = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
          if (lmin > -PMX_EPS) { found = true; break; }    // src/barycoord_pmmg.c:102-107
          if (step >= A.max_walk) break;
          if (FAR && (t.nb[0] | t.nb[1] | t.nb[2] | t.nb[3]) < 0) t = A.tets[cur];   // far fields
          const int next = exact_next(t, lam, ring, cur);
          if (!next) break;
          t = A.tets[next];
          cur = next;
          if (t.v[0] <= 0) break;
          step++;
#pragma unroll
          for (int l = 0; l < 4; l++) P[l] = ld3(A.xyz, t.v[l]);
        }
      }
    }
  }
  if constexpr (LAYOUT == LAYOUT_GEN) {       // S known at run time only: per-lane stores
    if (step != 0) walk_finish<LAYOUT, S, TIES>(A, i, p, found, step, cur, t, lam, s_cnt, s_sum, s_max, s_min);
  } else {
    walk_finish_wave<LAYOUT, S, TIES>(A, i, p, found, step, cur, t, lam, s_cnt, s_sum, s_max, s_min);
  }
  wave_stats_w(A.wstats + (b * blockDim.x + threadIdx.x) / 64, s_cnt, s_sum, s_max, s_min);
}

// exp 6: walk on the 32-B records although the compact ones are there
template <int LAYOUT, int S>
static void launch_walk_t(const VolArgs &a, int64_t nb, hipStream_t s, bool pointmap) {
  const dim3 g((unsigned)nb), bl(256);
  const bool cw = a.wrec && a.exp != 6;
  if (pointmap) {
    // point-map starts: the compact records' far fields always resolvable
    if (a.ref_walk) {
      if (a.inline_ties) hipLaunchKernelGGL((k_walk<LAYOUT, S, true, true>), g, bl, 0, s, a);
      else hipLaunchKernelGGL((k_walk<LAYOUT, S, false, true>), g, bl, 0, s, a);
    } else if (cw) {
      if (a.inline_ties) hipLaunchKernelGGL((k_walks<LAYOUT, S, true, true, true, true>), g, bl, 0, s, a);
      else hipLaunchKernelGGL((k_walks<LAYOUT, S, false, true, true, true>), g, bl, 0, s, a);
    } else {
      if (a.inline_ties) hipLaunchKernelGGL((k_walks<LAYOUT, S, true, false, false, true>), g, bl, 0, s, a);
      else hipLaunchKernelGGL((k_walks<LAYOUT, S, false, false, false, true>), g, bl, 0, s, a);
    }
    return;
  }
  if (a.ref_walk) {
    if (a.inline_ties) hipLaunchKernelGGL((k_walk<LAYOUT, S, true>), g, bl, 0, s, a);
    else hipLaunchKernelGGL((k_walk<LAYOUT, S, false>), g, bl, 0, s, a);
  } else if (cw) {
    if (a.inline_ties && a.far) hipLaunchKernelGGL((k_walks<LAYOUT, S, true, true, true>), g, bl, 0, s, a);
    else if (a.inline_ties) hipLaunchKernelGGL((k_walks<LAYOUT, S, true, true, false>), g, bl, 0, s, a);
    else if (a.far) hipLaunchKernelGGL((k_walks<LAYOUT, S, false, true, true>), g, bl, 0, s, a);
    else hipLaunchKernelGGL((k_walks<LAYOUT, S, false, true, false>), g, bl, 0, s, a);
  } else {
    // (the 32-B records have no far fields)
    if (a.inline_ties) hipLaunchKernelGGL((k_walks<LAYOUT, S, true, false, false>), g, bl, 0, s, a);
    else hipLaunchKernelGGL((k_walks<LAYOUT, S, false, false, false>), g, bl, 0, s, a);
  }
}

void launch_walk(const VolArgs &a, hipStream_t s, bool pointmap) {
  const int64_t nb = (a.nlist + 255) / 256;
  if (nb < 1) return;
  int S = 0;
  const int lay = walk_layout(a.sd, &S);
  if (lay == LAYOUT_ANI) return launch_walk_t<LAYOUT_ANI, 6>(a, nb, s, pointmap);
  if (lay == LAYOUT_ISO) {
    switch (S) {
      case 1: return launch_walk_t<LAYOUT_ISO, 1>(a, nb, s, pointmap);
      case 2: return launch_walk_t<LAYOUT_ISO, 2>(a, nb, s, pointmap);
      case 3: return launch_walk_t<LAYOUT_ISO, 3>(a, nb, s, pointmap);
      case 4: return launch_walk_t<LAYOUT_ISO, 4>(a, nb, s, pointmap);
      case 5: return launch_walk_t<LAYOUT_ISO, 5>(a, nb, s, pointmap);
      case 6: return launch_walk_t<LAYOUT_ISO, 6>(a, nb, s, pointmap);
      case 7: return launch_walk_t<LAYOUT_ISO, 7>(a, nb, s, pointmap);
      default: return launch_walk_t<LAYOUT_ISO, 8>(a, nb, s, pointmap);
    }
  }
  launch_walk_t<LAYOUT_GEN, 0>(a, nb, s, pointmap);
}

// ---- PMX_RUN_SEQUENTIAL_VOLUME: the reference's own walk, replayed in order --
//
// The reference's volume walk (PMMG_locatePointVol, src/locate_pmmg.c:786-883)
// starts from the previous volume point's tet (src/interpmesh_pmmg.c:529,
// :606-607) and marks every tet it visits with mesh->base.  Its answer depends
// on that start only where several tets contain the point (ties), where the
// walk gets stuck (status -1 instead of 1) or where it steps into a deleted
// tet (it spins there until step > ne and returns the closest tet visited,
// :809-811, :846-851).  pmx_seq.hip's seq_replay sorts the points into the
// vertex loop's order; here:
//  * k_seqv_spec -- every volume point walks the reference's walk exactly
//    (stable ascending-lambda order, first unvisited neighbour, closest
//    tracking) from its predecessor's device-semantics tet; the visited set is
//    a 16-entry lane list, and a walk that outgrows it, gets stuck or meets a
//    deleted tet is left to the replay ("unsure");
//  * k_seqv_resolve -- one wavefront keeps every speculative result whose
//    start was the true one and that was sure, and walks the others again,
//    in order, on the reference's tet flags (base compare); a stuck one goes
//    to the exhaustive scan (k_fallback, one point, launched from the host).
#define SEQV_CAP 16

template <int CAP> struct SeqvRegVis {
  int vis[CAP];
  int nv = 0;
  bool over = false;
  __device__ bool visited(int t) const {
    bool h = false;
#pragma unroll
    for (int i = 0; i < CAP; i++) h |= (i < nv) & (vis[i] == t);
    return h;
  }
  __device__ void mark(int t) {
    if (nv >= CAP) { over = true; return; }
#pragma unroll
    for (int i = 0; i < CAP; i++)
      if (i == nv) vis[i] = t;
    nv++;
  }
};
// a larger private set in a global workspace (the overflow pass): an
// open-addressing hash of {tet, generation} entries -- the generation (the
// point's sequence position + 1) makes a stale entry of an earlier point an
// empty slot, so nothing is cleared between points; at most half full
struct SeqvHashVis {
  int2 *tab;
  int mask = 0, nv = 0, gen = 0;
  bool over = false;
  __device__ __forceinline__ unsigned slot0(int t) const { return ((unsigned)t * 2654435761u) & (unsigned)mask; }
  __device__ bool visited(int t) const {
    for (unsigned h = slot0(t);; h = (h + 1) & (unsigned)mask) {
      const int2 e = tab[h];
      if (e.y != gen) return false;
      if (e.x == t) return true;
    }
  }
  __device__ void mark(int t) {
    if (2 * (nv + 1) > mask + 1) { over = true; return; }
    for (unsigned h = slot0(t);; h = (h + 1) & (unsigned)mask) {
      const int2 e = tab[h];
      if (e.y != gen) { tab[h] = make_int2(t, gen); nv++; return; }
      if (e.x == t) return;
    }
  }
};
struct SeqvGlobVis {
  int *tf;
  int base;
  bool over = false;
  __device__ bool visited(int t) const {
    return __hip_atomic_load(tf + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == base;
  }
  __device__ void mark(int t) { __hip_atomic_store(tf + t, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// returns 1 found (k, lam: its barycentrics in vertex order), 2 stuck (k the
// last tet), 3 visited list overflow, 4 the deleted-tet spin (k = the closest
// visited tet, 0 if none; step = ne + 1); ctet/lam of the closest for 4
template <class VS>
__device__ int ref_walk(const VolArgs &A, VS &vs, D3 p, int start, int &k, double lam[4], int &step) {
  int cur = start > 0 ? start : 1;
  double cdist = 1.0e10;
  int ctet = 0;
  step = 0;
  while (step <= A.ne) {
    step++;
    const TetRec t = A.tets[cur];
    if (t.v[0] <= 0) {                              // !MG_EOK: the reference spins here
      step = (int)A.ne + 1;
      k = ctet;
      return 4;
    }
    vs.mark(cur);
    if (vs.over) return 3;
    const D3 P[4] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2]), ld3(A.xyz, t.v[3])};
    double l[4], vol;
    tet_lambda(P, p, l, &vol);
    double sv[4] = {l[0], l[1], l[2], l[3]};
    int si[4] = {0, 1, 2, 3};
    sort4(sv, si);
    const double d = fabs(sv[0]) * vol;             // PMMG_locatePointInTetra :454-458
    if (d < cdist) { cdist = d; ctet = cur; }
    if (sv[0] > -PMX_EPS) {
      k = cur;
#pragma unroll
      for (int f = 0; f < 4; f++) lam[f] = l[f];
      return 1;
    }
    int next = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int nb = sel4(t.nb, si[r]);
      if (!next && nb && !vs.visited(nb)) next = nb;
    }
    if (!next) { k = cur; return 2; }
    cur = next;
  }
  k = ctet;
  return 4;
}

// the closest tet's one-hot barycentrics (PMMG_barycoord3d_getClosest,
// src/barycoord_pmmg.c:371-404): nearest vertex, first on ties
__device__ void closest_vertex(const VolArgs &A, int k, D3 p, double lam[4]) {
  const TetRec t = A.tets[k];
  double best = 0.0;
  int it = 0;
  for (int l = 0; l < 4; l++) {
    const D3 c = ld3(A.xyz, t.v[l]);
    const double d0 = p.x - c.x, d1 = p.y - c.y, d2 = p.z - c.z;
    const double d = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    if (l == 0 || d < best) { best = d; it = l; }
  }
  for (int l = 0; l < 4; l++) lam[l] = (l == it) ? 1.0 : 0.0;
}

__device__ void seqv_finish(const VolArgs &A, int64_t i, int k, const double lam[4], int status, int steps) {
  A.elem[i] = k;
  A.status[i] = status;
  A.steps[i] = steps;
  if (k <= 0) return;                               // no tet at all: untouched
  const TetRec t = A.tets[k];
  const int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
  const unsigned wm = interp_bar<4>(A.sol, A.sd, v, lam, A.out + i * A.sd.S);
  A.wmask[i] = (uint8_t)(wm | A.const_bit);
}

__global__ __launch_bounds__(256) void k_seqv_spec(VolArgs A, SeqVolArgs S) {
  const int n = *S.nvseq;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const int i = S.vseq[j];
    const D3 p{A.q[3 * (int64_t)i], A.q[3 * (int64_t)i + 1], A.q[3 * (int64_t)i + 2]};
    SeqvRegVis<SEQV_CAP> vs;
    int k, step;
    double lam[4];
    const int r = ref_walk(A, vs, p, S.sstart[i], k, lam, step);
    A.start[i] = S.sstart[i];
    S.sure[i] = r == 1 ? 1 : r == 3 ? 2 : 0;       // 2: a longer walk, for the overflow pass
    if (r == 1) seqv_finish(A, i, k, lam, 1, step);
  }
}

// the walks that outgrew the lane list, again with a SEQV_OVF_CAP list in a
// global workspace (walks from the previous point's tet are long where the
// visit order jumps: ~2 % of C3's points walk more than 16 tets)
#define SEQV_OVF_CAP 4096            // hash slots per thread: walks of up to 2048 tets
#define SEQV_OVF_THREADS (4 * 64 * 256)    // 2 GB of hash tables (r06: 4x, C3 78 ms on 16384 threads)
__global__ __launch_bounds__(256) void k_seqv_ovf(VolArgs A, SeqVolArgs S, int *ws) {
  const int n = *S.nvseq;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  for (int j = tid; j < n; j += gridDim.x * blockDim.x) {
    const int i = S.vseq[j];
    if (S.sure[i] != 2) continue;
    const D3 p{A.q[3 * (int64_t)i], A.q[3 * (int64_t)i + 1], A.q[3 * (int64_t)i + 2]};
    SeqvHashVis vs;
    vs.tab = reinterpret_cast<int2 *>(ws) + (size_t)tid * SEQV_OVF_CAP;
    vs.mask = SEQV_OVF_CAP - 1;
    vs.gen = j + 1;
    int k, step;
    double lam[4];
    const int r = ref_walk(A, vs, p, S.sstart[i], k, lam, step);
    S.sure[i] = r == 1 ? 1 : 0;
    if (r == 1) seqv_finish(A, i, k, lam, 1, step);
  }
}

// the positions the replay must look at: a point whose speculative walk is
// not sure, or started from another tet than its predecessor's speculative
// result (ties, walks into deleted tets); position 0 starts from tet 1
__global__ __launch_bounds__(256) void k_seqv_flags(VolArgs A, SeqVolArgs S, int64_t nmax, uint8_t *flags) {
  const int n = *S.nvseq;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nmax; j += (int64_t)gridDim.x * blockDim.x) {
    bool bad = false;
    if (j < n) {
      const int i = S.vseq[j];
      const int want = j == 0 ? 1 : A.elem[S.vseq[j - 1]];
      bad = !(S.sure[i] && S.sstart[i] == want);
    }
    flags[j] = bad ? 1 : 0;
  }
}

// the replay: one lane, in visit order; ctl = {next position, its start (-1:
// the tet of the previous point, after a stuck walk the host resolved),
// state (0 done, 1 stuck: the host scans), the point}.  A position is looked
// at when it is a candidate (S.cand) or when its predecessor was replayed
// ("dirty"): every other point's speculative start is its predecessor's
// final tet, so its speculative result stands.  (r06 first version scanned
// all n positions with the wave: 0.40 s of C3's 0.65-s sequential step.)
__global__ __launch_bounds__(64) void k_seqv_resolve(VolArgs A, SeqVolArgs S) {
  if (threadIdx.x != 0) return;
  const int n = *S.nvseq;
  int j = S.ctl[0];
  int prev = S.ctl[1];
  if (j >= n) return;
  bool dirty = prev < 0;                         // resumed after a stuck walk
  if (prev < 0) prev = A.elem[S.vseq[j - 1]];
  const int nc = *S.ncand;
  int lo = 0, hi = nc;                           // first candidate >= j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.cand[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  int pos = lo;
  unsigned replays = 0;
  while (j < n) {
    if (!dirty) {
      while (pos < nc && S.cand[pos] < j) pos++;
      if (pos >= nc) break;                      // every later speculative result stands
      const int c = S.cand[pos];
      if (c > j) {
        prev = A.elem[S.vseq[c - 1]];
        j = c;
      }
    }
    const int i = S.vseq[j];
    if (S.sure[i] && S.sstart[i] == prev) {      // the speculative walk started right
      prev = A.elem[i];
      dirty = false;
      j++;
      continue;
    }
    const D3 p{A.q[3 * (int64_t)i], A.q[3 * (int64_t)i + 1], A.q[3 * (int64_t)i + 2]};
    SeqvGlobVis vs{S.tf, S.sbase[i]};
    int k, step;
    double lam[4];
    A.start[i] = prev;
    const int r = ref_walk(A, vs, p, prev, k, lam, step);
    replays++;
    if (r == 1) {
      seqv_finish(A, i, k, lam, 1, step);
    } else if (r == 4) {
      if (k > 0) closest_vertex(A, k, p, lam);
      seqv_finish(A, i, k, lam, 0, step);
    } else {                                      // stuck: the exhaustive scan
      A.steps[i] = -step;
      S.stk_list[0] = i;
      S.ctl[0] = j;
      S.ctl[2] = 1;
      S.ctl[3] = i;
      atomicAdd(S.nreplay, replays);
      return;
    }
    prev = k;
    dirty = true;
    j++;
  }
  S.ctl[0] = n;
  S.ctl[2] = 0;
  atomicAdd(S.nreplay, replays);
}

size_t seqv_ovf_ws_ints() { return (size_t)SEQV_OVF_THREADS * SEQV_OVF_CAP * 2; }
void launch_seqv_spec(const VolArgs &a, const SeqVolArgs &s, int64_t nmax, int *ws, hipStream_t st) {
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>((nmax + 255) / 256, 65536));
  hipLaunchKernelGGL(k_seqv_spec, dim3((unsigned)nb), dim3(256), 0, st, a, s);
  hipLaunchKernelGGL(k_seqv_ovf, dim3(SEQV_OVF_THREADS / 256), dim3(256), 0, st, a, s, ws);
}
void launch_seqv_flags(const VolArgs &a, const SeqVolArgs &s, int64_t nmax, uint8_t *flags, hipStream_t st) {
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>((nmax + 255) / 256, 65536));
  hipLaunchKernelGGL(k_seqv_flags, dim3((unsigned)nb), dim3(256), 0, st, a, s, nmax, flags);
}
void launch_seqv_resolve(const VolArgs &a, const SeqVolArgs &s, hipStream_t st) {
  hipLaunchKernelGGL(k_seqv_resolve, dim3(1), dim3(64), 0, st, a, s);
}
