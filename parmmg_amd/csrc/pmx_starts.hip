// pmx_starts.hip -- per-background derived data and where a walk starts, on
// gfx950: the kernels and the functions that launch them.
//
// k_bg_derive        per-background derived data, one launch: fixed-point grid
//                    coordinates of the old vertices (hint centroids) and the
//                    unit normals of the boundary trias
//                    (PMMG_precompute_triaNormals, src/locate_pmmg.c:68-90)
// k_hint_build       uniform grid over the background bbox, cell -> a sampled
//                    tet whose centroid falls in it (the walk start)
// k_vmin_owner,      the vertex-owner hint sample: one tet per vertex, in
// k_owner_flags,     vertex order (PMX_HINT_SAMPLE_ORDER=2)
// k_owner_gather
// k_pmap_tets,       PMX_RUN_POINTMAP: the first-incident-element maps of a
// k_pmap_trias       background (PMMG_locate_setStart, src/locate_pmmg.c:931-986)
// The walks that start there are pmx_walk.hip (volume) and pmx_bdy.hip (surface).
#include <algorithm>
#include <hipcub/hipcub.hpp>
#include "pmx_device.h"
#include "pmx_kernels.h"
#include "pmx_transfer.h"
#include "pmx_host.h"

// ---- per-background derived data -----------------------------------------------

// a vertex's grid coordinates in fixed point (k_hint_build's centroids):
// q = (x - lo) * inv * 2^qf, clamped to [0, dim * 2^qf - 1] (21 bits per
// axis), packed x | y << 21 | z << 42
__device__ __forceinline__ unsigned long long quant_xyz(const double *c, const GridDesc &g) {
  unsigned long long r = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double t = (c[a] - g.lo[a]) * g.inv[a] * (double)(1 << g.qf[a]);
    const long long hi = ((long long)g.dim[a] << g.qf[a]) - 1;
    const long long u = !(t > 0.0) ? 0 : (t >= (double)hi ? hi : (long long)t);
    r |= (unsigned long long)u << (21 * a);
  }
  return r;
}

// Blocks [0, nbv) quantise the vertices, 256 pairs of rows (12 KB) per
// block iteration: three fully coalesced 16-B loads per thread into LDS, each
// thread then takes its two rows from LDS (r05: two rows per thread straight
// from HBM -- three 16-B loads at a 48-B lane stride -- ran at 4.2 TB/s,
// 0.128 ms at C3).  Blocks [nbv, nbv + nbt) form the tria normals.
__global__ __launch_bounds__(256) void k_bg_derive(const double *__restrict__ xyz, int64_t np, GridDesc g,
                                                   unsigned long long *__restrict__ q,
                                                   const TriRec *__restrict__ tris, int64_t nt,
                                                   Pt4 *__restrict__ trn, int nbv) {
  __shared__ double2 sh[3 * 256];
  auto quant = [&](const double *c) { return quant_xyz(c, g); };
  if ((int)blockIdx.x < nbv) {
    const int64_t npair = (np + 2) / 2;         // rows 0 .. np, two per pair
    const int64_t nfull = (np + 1) / 2;         // pairs with both rows
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < npair; b0 += (int64_t)nbv * 256) {
      const int64_t m = b0 + threadIdx.x;
      if (b0 + 256 <= nfull) {                  // block-uniform: a whole chunk
        const double2 *p = reinterpret_cast<const double2 *>(xyz + 6 * b0);
        sh[threadIdx.x] = p[threadIdx.x];
        sh[threadIdx.x + 256] = p[threadIdx.x + 256];
        sh[threadIdx.x + 512] = p[threadIdx.x + 512];
        __syncthreads();
        const double2 a = sh[3 * threadIdx.x], b = sh[3 * threadIdx.x + 1], c = sh[3 * threadIdx.x + 2];
        __syncthreads();
        const double c0[3] = {a.x, a.y, b.x}, c1[3] = {b.y, c.x, c.y};
        reinterpret_cast<ulonglong2 *>(q)[m] = make_ulonglong2(quant(c0), quant(c1));
      } else if (m < npair) {                   // the tail
        if (2 * m + 1 <= np) {
          const double2 *p = reinterpret_cast<const double2 *>(xyz + 6 * m);
          const double2 a = p[0], b = p[1], c = p[2];
          const double c0[3] = {a.x, a.y, b.x}, c1[3] = {b.y, c.x, c.y};
          reinterpret_cast<ulonglong2 *>(q)[m] = make_ulonglong2(quant(c0), quant(c1));
        } else {
          const double c0[3] = {xyz[6 * m], xyz[6 * m + 1], xyz[6 * m + 2]};
          q[2 * m] = quant(c0);
        }
      }
    }
    return;
  }
  const int64_t st = (int64_t)(gridDim.x - nbv) * blockDim.x;
  for (int64_t k = 1 + (int64_t)(blockIdx.x - nbv) * blockDim.x + threadIdx.x; k <= nt; k += st) {
    const TriRec t = tris[k];
    if (t.v[0] <= 0) { trn[k] = Pt4{0, 0, 0, 0}; continue; }
    const D3 n = nonunit_normal(ld3(xyz, t.v[0]), ld3(xyz, t.v[1]), ld3(xyz, t.v[2]));
    const double a = sqrt(n.x * n.x + n.y * n.y + n.z * n.z);
    const double dd = 1.0 / a;
    trn[k] = Pt4{n.x * dd, n.y * dd, n.z * dd, a};
  }
}
void launch_bg_derive(const double *xyz, int64_t np, GridDesc g, unsigned long long *xyzq,
                      const TriRec *tris, int64_t nt, Pt4 *trn, hipStream_t s) {
  const int64_t npair = np > 0 ? (np + 2) / 2 : 0;
  const int nbv = (int)std::min<int64_t>((npair + 255) / 256, 8192);
  const int nbt = (int)std::min<int64_t>((nt + 255) / 256, 4096);
  if (nbv + nbt < 1) return;
  hipLaunchKernelGGL(k_bg_derive, dim3((unsigned)(nbv + nbt)), dim3(256), 0, s, xyz, np, g, xyzq, tris, nt, trn,
                     nbv);
}

// ---- hint grid ---------------------------------------------------------------------

// One sample per thread; XCD-aware block order: each XCD's L2 serves a
// contiguous range of samples, i.e. neighbouring tets sharing vertices.  The
// centroid's cell comes from the vertices' fixed-point grid coordinates (one
// 8-B gather per vertex, integer sums and a shift, no FP; r01 same-box A/B on
// C3: 0.197 ms against 0.295 ms from the double coordinates).  Plain store:
// any sampled tet of the cell is a valid start, the located tet does not
// depend on the start (unique containing tet, or the canonical min-index tet
// of a tie, see canonical_tet).
// the cell of a tet's centroid from its vertices' fixed-point coordinates
__device__ __forceinline__ int64_t hint_cell(unsigned long long a, unsigned long long b, unsigned long long c,
                                             unsigned long long d, const GridDesc &g) {
  const unsigned long long M = (1ull << 21) - 1;
  int cq[3];
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const int sh = 21 * ax;
    const unsigned s4 = (unsigned)((a >> sh) & M) + (unsigned)((b >> sh) & M) +
                        (unsigned)((c >> sh) & M) + (unsigned)((d >> sh) & M);
    cq[ax] = min((int)(s4 >> (g.qf[ax] + 2)), g.dim[ax] - 1);
  }
  return gcell(g, cq[0], cq[1], cq[2]);
}

template <bool PACKED>
__global__ __launch_bounds__(256) void k_hint_build(const int4 *__restrict__ packed, const int *__restrict__ kidx,
                                                    const TetRec *__restrict__ tets, int64_t n,
                                                    int stride, int *__restrict__ grid, GridDesc g,
                                                    const unsigned long long *__restrict__ xyzq) {
  const int64_t t = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  if (t >= n) return;
  // the packed sample in cell order carries its tet indices (kidx)
  const int64_t k = (PACKED && kidx) ? (int64_t)kidx[t] : 1 + t * stride;
  const int4 v = PACKED ? packed[t] : *reinterpret_cast<const int4 *>(tets + k);
  if (v.x <= 0) return;
  grid[hint_cell(xyzq[v.x], xyzq[v.y], xyzq[v.z], xyzq[v.w], g)] = (int)k;
}
void launch_hint_build(const int4 *packed, const int *kidx, const TetRec *tets, int64_t ne, int stride, int *grid,
                       GridDesc g, const unsigned long long *xyzq, hipStream_t s, int64_t nsamp) {
  const int64_t n = nsamp >= 0 ? nsamp : (ne + stride - 1) / stride;   // nsamp < 0: every stride-th tet
  if (n < 1) return;
  const int64_t nb = (n + 255) / 256;
  if (packed)
    hipLaunchKernelGGL(k_hint_build<true>, dim3((unsigned)nb), dim3(256), 0, s, packed, kidx, tets, n, stride, grid,
                       g, xyzq);
  else
    hipLaunchKernelGGL(k_hint_build<false>, dim3((unsigned)nb), dim3(256), 0, s, packed, kidx, tets, n, stride, grid,
                       g, xyzq);
}

// The vertex-owner sample (r05): one tet per vertex -- the smallest tet
// among those whose smallest vertex it is -- in vertex order.  Like the
// every-4th-tet sample it is connectivity only, but it covers space whatever
// the tet numbering (a random numbering's every-4th-tet sample leaves a
// Poisson share of the cells empty), and it has one entry per vertex instead
// of ne / 4.
// (a lane whose left neighbour -- the previous tet -- has the same smallest
// vertex skips its atomic: a coherent numbering puts a vertex's tets next to
// each other, and same-address atomics serialise; r05: 3.6 -> see DESIGN)
__global__ __launch_bounds__(256) void k_vmin_owner(const TetRec *__restrict__ tets, int64_t ne,
                                                    unsigned *__restrict__ owner) {
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  const int64_t nit = (ne + st - 1) / st;           // uniform trip count (the shuffle below)
  for (int64_t it = 0; it < nit; it++) {
    const int64_t k = 1 + it * st + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int m = -1;
    if (k <= ne) {
      const int4 v = *reinterpret_cast<const int4 *>(tets + k);
      if (v.x > 0) m = min(min(v.x, v.y), min(v.z, v.w));
    }
    const int ml = __shfl_up(m, 1, 64);
    const bool first = (threadIdx.x & 63) == 0 || ml != m;
    if (m > 0 && first) atomicMin(owner + m, (unsigned)k);
  }
}
__global__ __launch_bounds__(256) void k_owner_flags(const unsigned *__restrict__ owner, int64_t np,
                                                     int *__restrict__ flag) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= np; v += (int64_t)gridDim.x * blockDim.x)
    flag[v] = (v >= 1 && owner[v] != 0xffffffffu) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_owner_gather(const unsigned *__restrict__ owner, const int *__restrict__ flag,
                                                      const int *__restrict__ pos, int64_t np,
                                                      const TetRec *__restrict__ tets, int4 *__restrict__ out,
                                                      int *__restrict__ kidx, unsigned *__restrict__ count) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= np; v += (int64_t)gridDim.x * blockDim.x) {
    if (flag[v]) {
      const int k = (int)owner[v];
      out[pos[v]] = *reinterpret_cast<const int4 *>(tets + k);
      kidx[pos[v]] = k;
    }
    if (v == np) *count = (unsigned)(pos[v] + flag[v]);
  }
}
size_t owner_scan_temp_bytes(int64_t np) {
  size_t bytes = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int *)nullptr, (int *)nullptr, (int)(np + 1));
  return bytes;
}
bool launch_owner_sample(const TetRec *tets, int64_t ne, int64_t np, unsigned *owner, int *flag, int *pos,
                         int4 *out, int *kidx, unsigned *d_count, unsigned *h_count, void *tmp, size_t tmp_bytes,
                         hipStream_t s) {
  if (hipMemsetAsync(owner, 0xff, (size_t)(np + 1) * sizeof(unsigned), s) != hipSuccess) return false;
  const unsigned nbt = pmx_grid(ne, 65536), nbv = pmx_grid(np + 1, 65536);
  hipLaunchKernelGGL(k_vmin_owner, dim3(nbt), dim3(256), 0, s, tets, ne, owner);
  hipLaunchKernelGGL(k_owner_flags, dim3(nbv), dim3(256), 0, s, (const unsigned *)owner, np, flag);
  if (hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, (const int *)flag, pos, (int)(np + 1), s) != hipSuccess)
    return false;
  hipLaunchKernelGGL(k_owner_gather, dim3(nbv), dim3(256), 0, s, (const unsigned *)owner,
                     (const int *)flag, (const int *)pos, np, tets, out, kidx, d_count);
  if (hipMemcpyAsync(h_count, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess) return false;
  return hipGetLastError() == hipSuccess;
}

// ---- PMX_RUN_POINTMAP: the first-incident-element maps ---------------------
//
// vmap[p] = min{k : tets[k].v[0] > 0, p in tets[k].v}, tmap[p] = min{k : p in
// tris[k].v} -- what the reference's loops leave in ppt->s / ppt->tmp
// (PMMG_locate_setStart keeps the first index that reaches a vertex).  The
// exact minimum needs atomicMin: a plain store would make the start, and with
// it the surface answers, vary from run to run.  A lane reads the slot first
// and issues the atomic only when its element is smaller (the slots only ever
// decrease, so a stale read costs an atomic, never the minimum).  Measured at
// C3: the read filters 70 % of the 4 ne candidates in the lattice numbering
// (the tets in flight together around a vertex's first cell all issue), 90 %
// in a shuffled one.  The atomics issued are counted
// per wave (cnt), one add per wave that issued any.
__device__ __forceinline__ void pmap_min(unsigned *__restrict__ map, int v, int64_t np, unsigned k,
                                         unsigned &issued) {
  if (v < 1 || (int64_t)v > np) return;
  if (__hip_atomic_load(map + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > k) {
    atomicMin(map + v, k);
    issued++;
  }
}
__device__ __forceinline__ void pmap_count(unsigned issued, unsigned *cnt) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) issued += __shfl_xor(issued, o, 64);
  if ((threadIdx.x & 63) == 0 && issued) atomicAdd(cnt, issued);
}
__global__ __launch_bounds__(256) void k_pmap_tets(const TetRec *__restrict__ tets, int64_t ne, int64_t np,
                                                   unsigned *__restrict__ vmap, unsigned *__restrict__ cnt) {
  unsigned issued = 0;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= ne; k += st) {
    const int4 v = *reinterpret_cast<const int4 *>(tets + k);
    if (v.x <= 0) continue;                              // deleted tet
    pmap_min(vmap, v.x, np, (unsigned)k, issued);
    pmap_min(vmap, v.y, np, (unsigned)k, issued);
    pmap_min(vmap, v.z, np, (unsigned)k, issued);
    pmap_min(vmap, v.w, np, (unsigned)k, issued);
  }
  pmap_count(issued, cnt);
}
__global__ __launch_bounds__(256) void k_pmap_trias(const TriRec *__restrict__ tris, int64_t nt, int64_t np,
                                                    unsigned *__restrict__ tmap, unsigned *__restrict__ cnt) {
  unsigned issued = 0;
  const int64_t st = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nt; k += st) {
    const int4 v = *reinterpret_cast<const int4 *>(tris + k);    // v[0..2], pad
    pmap_min(tmap, v.x, np, (unsigned)k, issued);
    pmap_min(tmap, v.y, np, (unsigned)k, issued);
    pmap_min(tmap, v.z, np, (unsigned)k, issued);
  }
  pmap_count(issued, cnt);
}
void launch_pmap_build(const TetRec *tets, int64_t ne, const TriRec *tris, int64_t nt, int64_t np,
                       unsigned *map, unsigned *cnt, hipStream_t s) {
  unsigned *vmap = map, *tmap = map + (np + 1);
  hipMemsetAsync(map, 0xff, (size_t)(2 * (np + 1)) * sizeof(unsigned), s);
  hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned), s);
  const int64_t nbt = std::min<int64_t>((ne + 255) / 256, 65536);
  const int64_t nbs = std::min<int64_t>((nt + 255) / 256, 4096);
  if (nbt > 0) hipLaunchKernelGGL(k_pmap_tets, dim3((unsigned)nbt), dim3(256), 0, s, tets, ne, np, vmap, cnt);
  if (nbs > 0) hipLaunchKernelGGL(k_pmap_trias, dim3((unsigned)nbs), dim3(256), 0, s, tris, nt, np, tmap, cnt + 1);
}
