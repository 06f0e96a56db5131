// pmx_fallback.hip -- what the volume walk leaves behind, on gfx950: the
// near-face ties and the exhaustive scan of the stuck points.
//
// k_ties             near-face ties: canonical (smallest-index) containing tet
// k_fallback         LDS-staged exhaustive scan (smallest containing tet
//                    index == the reference's first hit in index order,
//                    src/locate_pmmg.c:737-770), closest tet (argmin of
//                    |lambda_min|*vol, src/barycoord_pmmg.c:371-404) and the
//                    interpolation of the scanned points, phases separated by
//                    a grid barrier that reports a timeout instead of hiding it
// The production walk itself is pmx_walk.hip.
#include <algorithm>
#include "pmx_device.h"
#include "pmx_kernels.h"
#include "pmx_transfer.h"

// ---- ties -----------------------------------------------------------------------

// A point with some lambda_f < TIE_NEAR in its tet may also satisfy the
// reference's inside test (lambda_min > -1e-6, src/barycoord_pmmg.c:102-107)
// in the neighbours across those faces (face / edge / vertex ties).  The
// reference returns whichever its path reaches first; the device returns the
// smallest index of the connected set of containing tets, so the answer is
// independent of the start tet (and equals the exhaustive scan's first hit).
// lambda_f < 10*EPS admits neighbours up to 10x larger across face f: a tie
// across a sharper size jump is still a containing tet, only not canonical
#define TIE_NEAR 1.e-5
#define TIE_CAP 48
__device__ __noinline__ int canonical_tet(const TetRec *tets, const double *xyz, int k0, D3 p) {
  int vis[TIE_CAP], inq[TIE_CAP];
  int nv = 0, nq = 0, head = 0, best = k0;
  vis[nv++] = k0;
  inq[nq++] = k0;
  while (head < nq) {
    int k = inq[head++];
    TetRec t = tets[k];
    D3 P[4] = {ld3(xyz, t.v[0]), ld3(xyz, t.v[1]), ld3(xyz, t.v[2]), ld3(xyz, t.v[3])};
    double lam[4], vol;
    tet_lambda(P, p, lam, &vol);
    for (int f = 0; f < 4; f++) {
      int nb = t.nb[f];
      if (!nb || !(lam[f] < TIE_NEAR)) continue;
      bool seen = false;
      for (int q = 0; q < nv; q++) seen |= (vis[q] == nb);
      if (seen) continue;
      if (nv == TIE_CAP) return -1;
      vis[nv++] = nb;
      TetRec u = tets[nb];
      if (u.v[0] <= 0) continue;
      D3 Q[4] = {ld3(xyz, u.v[0]), ld3(xyz, u.v[1]), ld3(xyz, u.v[2]), ld3(xyz, u.v[3])};
      double mu[4], vu;
      tet_lambda(Q, p, mu, &vu);
      if (fmin(fmin(mu[0], mu[1]), fmin(mu[2], mu[3])) > -PMX_EPS) {
        if (nq == TIE_CAP) return -1;
        inq[nq++] = nb;
        best = nb < best ? nb : best;
      }
    }
  }
  return best;
}

__device__ void d_ties(const VolArgs &A, unsigned bid, unsigned nblk) {
  const unsigned n = *A.tie_count;
  for (unsigned j = bid * blockDim.x + threadIdx.x; j < n; j += nblk * blockDim.x) {
    int2 e = A.tie_list[j];
    const int64_t i = e.x;
    const D3 p = ld3(A.q, (int)i);
    int kc = canonical_tet(A.tets, A.xyz, e.y, p);
    if (kc < 0) {                                   // tie set too large: scan
      unsigned slot = atomicAdd(A.stuck_count, 1u);
      A.stuck_list[slot] = (int)i;
      A.found[slot] = 0x7fffffff;
      A.bestk[slot] = 0x7fffffff;
      A.best[slot] = ~0ull;
      A.steps[i] = -A.steps[i];
      continue;
    }
    TetRec t = A.tets[kc];
    int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
    D3 P[4] = {ld3(A.xyz, v[0]), ld3(A.xyz, v[1]), ld3(A.xyz, v[2]), ld3(A.xyz, v[3])};
    double lam[4], vol;
    tet_lambda(P, p, lam, &vol);
    A.elem[i] = kc;
    A.status[i] = 1;
    unsigned wm = interp_bar<4>(A.sol, A.sd, v, lam, A.out + i * A.sd.S);
    A.wmask[i] = (uint8_t)(wm | A.const_bit);
  }
}

// ---- exhaustive fallback ---------------------------------------------------

#define EXH_CHUNK 256

// smallest tet index containing each stuck point (bbox prefilter, exact test)
__device__ void d_exh_find(const ExhArgs &A, unsigned bid, unsigned nblk) {
  __shared__ D3 sp[EXH_CHUNK];
  const unsigned n = *A.count;
  for (unsigned c0 = 0; c0 < n; c0 += EXH_CHUNK) {
    unsigned m = min((unsigned)EXH_CHUNK, n - c0);
    __syncthreads();
    for (unsigned j = threadIdx.x; j < m; j += blockDim.x) sp[j] = ld3(A.q, A.list[c0 + j]);
    __syncthreads();
    for (int64_t k = 1 + (int64_t)bid * blockDim.x + threadIdx.x; k <= A.ne;
         k += (int64_t)nblk * blockDim.x) {
      TetRec t = A.tets[k];
      if (t.v[0] <= 0) continue;
      D3 P[4] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2]), ld3(A.xyz, t.v[3])};
      double lo[3] = {P[0].x, P[0].y, P[0].z}, hi[3] = {P[0].x, P[0].y, P[0].z};
#pragma unroll
      for (int l = 1; l < 4; l++) {
        lo[0] = fmin(lo[0], P[l].x); hi[0] = fmax(hi[0], P[l].x);
        lo[1] = fmin(lo[1], P[l].y); hi[1] = fmax(hi[1], P[l].y);
        lo[2] = fmin(lo[2], P[l].z); hi[2] = fmax(hi[2], P[l].z);
      }
      // lambda_i >= -1e-6 for all i keeps the point within 3e-6 * extent of
      // the bbox; 1e-5 * max extent is a safe margin
      double ext = fmax(hi[0] - lo[0], fmax(hi[1] - lo[1], hi[2] - lo[2]));
      double mg = 1.e-5 * ext;
      for (unsigned j = 0; j < m; j++) {
        D3 p = sp[j];
        if (p.x < lo[0] - mg || p.x > hi[0] + mg || p.y < lo[1] - mg || p.y > hi[1] + mg ||
            p.z < lo[2] - mg || p.z > hi[2] + mg)
          continue;
        double lam[4], vol;
        tet_lambda(P, p, lam, &vol);
        double mn = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
        if (mn > -PMX_EPS) atomicMin(&A.found[c0 + j], (int)k);
      }
    }
  }
}

// argmin over all tets of |lambda_min| * vol for points found nowhere
__device__ void d_exh_closest(const ExhArgs &A, int pass, unsigned bid, unsigned nblk) {
  __shared__ D3 sp[EXH_CHUNK];
  __shared__ int act[EXH_CHUNK];
  const unsigned n = *A.count;
  for (unsigned c0 = 0; c0 < n; c0 += EXH_CHUNK) {
    unsigned m = min((unsigned)EXH_CHUNK, n - c0);
    __syncthreads();
    for (unsigned j = threadIdx.x; j < m; j += blockDim.x) {
      sp[j] = ld3(A.q, A.list[c0 + j]);
      act[j] = (A.found[c0 + j] == 0x7fffffff);
    }
    __syncthreads();
    for (int64_t k = 1 + (int64_t)bid * blockDim.x + threadIdx.x; k <= A.ne;
         k += (int64_t)nblk * blockDim.x) {
      TetRec t = A.tets[k];
      if (t.v[0] <= 0) continue;
      D3 P[4] = {ld3(A.xyz, t.v[0]), ld3(A.xyz, t.v[1]), ld3(A.xyz, t.v[2]), ld3(A.xyz, t.v[3])};
      for (unsigned j = 0; j < m; j++) {
        if (!act[j]) continue;
        double lam[4], vol;
        tet_lambda(P, sp[j], lam, &vol);
        double mn = fmin(fmin(lam[0], lam[1]), fmin(lam[2], lam[3]));
        double d = fabs(mn) * vol;                 // src/locate_pmmg.c:455-458
        unsigned long long bits = (unsigned long long)__double_as_longlong(d);
        if (pass == 0) atomicMin(&A.best[c0 + j], bits);
        else if (bits == A.best[c0 + j]) atomicMin(&A.bestk[c0 + j], (int)k);
      }
    }
  }
}

__device__ void d_exh_finish(const ExhArgs &A, const VolArgs &V, unsigned bid, unsigned nblk) {
  const unsigned n = *A.count;
  for (unsigned j = bid * blockDim.x + threadIdx.x; j < n; j += nblk * blockDim.x) {
    int64_t i = A.list[j];
    const D3 p = ld3(A.q, (int)i);
    int k = A.found[j];
    int st = 1;
    double phi[4];
    if (k == 0x7fffffff) {
      k = A.bestk[j];
      st = 0;
    }
    if (k == 0x7fffffff) {                          // no valid tet at all: left untouched
      V.elem[i] = 0;
      V.status[i] = 0;
      continue;
    }
    TetRec t = A.tets[k];
    int v[4] = {t.v[0], t.v[1], t.v[2], t.v[3]};
    D3 P[4] = {ld3(A.xyz, v[0]), ld3(A.xyz, v[1]), ld3(A.xyz, v[2]), ld3(A.xyz, v[3])};
    if (st) {
      double vol;
      tet_lambda(P, p, phi, &vol);
    } else {
      // PMMG_barycoord3d_getClosest: nearest vertex, first on ties
      double best = 0.0;
      int it = 0;
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double d0 = p.x - P[l].x, d1 = p.y - P[l].y, d2 = p.z - P[l].z;
        double d = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (l == 0 || d < best) { best = d; it = l; }
      }
#pragma unroll
      for (int l = 0; l < 4; l++) phi[l] = (l == it) ? 1.0 : 0.0;
    }
    V.elem[i] = k;
    V.status[i] = st ? -1 : 0;
    V.steps[i] = V.steps[i] - 1;
    unsigned wm = interp_bar<4>(V.sol, V.sd, v, phi, V.out + i * V.sd.S);
    V.wmask[i] = (uint8_t)(V.wmask[i] | wm);
  }
}

// ---- fused fallback -------------------------------------------------------------
//
// Exhaustive scan (find, closest value, closest index) and the final
// interpolation of the scanned points in ONE launch (four launches that almost
// always found nothing to do cost ~4.5 us each).  The launch reads the
// counters and leaves, or runs the phases separated by a grid barrier
// (MI355X_MICROARCH.md "barrier-counter": release fence + waitcnt before the
// arrive, relaxed agent-scope poll, acquire fence after).  Its grid is sized
// on the host from the occupancy query so that every workgroup is co-resident
// even beside another context's fallback (fallback_coresident_blocks); should
// a barrier still time out, the workgroup records PMX_DERR_BARRIER in the
// step's error word and every later phase is skipped, and the host turns that
// into a failed call (pmx_synchronize / pmx_download) -- never a silent result.

__device__ __forceinline__ unsigned ld_agent(const unsigned *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// false when the wait gave up (the error word is set then)
__device__ bool grid_barrier(unsigned *bar, unsigned target, unsigned *err, long spin_limit) {
  __shared__ int s_ok;
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    atomicAdd(bar, 1u);
    long it = 0;
    while (ld_agent(bar) < target && ld_agent(err) == 0u && it < spin_limit) {
      __builtin_amdgcn_s_sleep(2);
      it++;
    }
    const bool ok = ld_agent(bar) >= target && ld_agent(err) == 0u;
    if (!ok) atomicOr(err, PMX_DERR_BARRIER);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_ok = ok ? 1 : 0;
  }
  __syncthreads();
  return s_ok != 0;
}

// The ties (canonical tet BFS, independent per point) are a launch of their
// own: a step with ties but no stuck point (the common case: 71 ties at C3)
// then needs no grid barrier, so its fallback never waits for co-residency
// behind another context's walk (C4: two groups per GPU).  The tie launch may
// append points to the stuck list; the kernel boundary orders that.
__global__ __launch_bounds__(256) void k_ties(VolArgs V) {
  if (ld_agent(V.tie_count) == 0) return;
  d_ties(V, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void k_fallback(ExhArgs E, VolArgs V) {
  const unsigned nb = gridDim.x, b = blockIdx.x;
  unsigned *bar = V.stuck_count + 4;           // counts[4], zeroed by the prologue
  unsigned *err = V.stuck_count + PMX_CNT_ERR;
  if (ld_agent(V.stuck_count) == 0) return;
  d_exh_find(E, b, nb);
  if (!grid_barrier(bar, nb, err, E.spin_limit)) return;
  d_exh_closest(E, 0, b, nb);
  if (!grid_barrier(bar, 2 * nb, err, E.spin_limit)) return;
  d_exh_closest(E, 1, b, nb);
  if (!grid_barrier(bar, 3 * nb, err, E.spin_limit)) return;
  d_exh_finish(E, V, b, nb);
}

int fallback_coresident_blocks(int device, int share) {
  int cus = 0, per_cu = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(k_fallback),
                                                   256, 0) != hipSuccess)
    return 0;
  const long cap = (long)cus * per_cu / std::max(1, share);
  return (int)std::min<long>(256, cap);
}

void launch_exhaustive(const ExhArgs &e, const VolArgs &v, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_ties, dim3(64), dim3(256), 0, s, v);
  hipLaunchKernelGGL(k_fallback, dim3((unsigned)std::max(1, blocks)), dim3(256), 0, s, e, v);
}
