// pmx_fans.hip -- the node -> trias fans of the background's surface on gfx950.
//
// The content of PMMG_precompute_nodeTrias (src/locate_pmmg.c:134-195): per
// boundary vertex its incident boundary trias in increasing tria index, and
// the fan sizes the point flags start from.  Rebuilt by every step that
// rebuilds the background's derived data -- the reference builds it inside
// PMMG_interpMetricsAndFields (src/interpmesh_pmmg.c:707).  ntlist holds the
// fans, ntrange[3 k + l] the fan [lo, hi) of vertex l of tria k: the surface
// kernels always reach a vertex through a tria that holds it, so there are no
// per-vertex offsets over np.  Three builds with the same output:
//  * by rotation through the tria adjacency (r05, below): a closed manifold
//    surface, which the upload checks (check_fans);
//  * a counting sort over the vertex ids -- count -> exclusive scan over np ->
//    fill at the vertex's offset (slot by atomic, order arbitrary) -> the
//    slot-0 writer sorts its fan (a few entries): its arrays are np-sized;
//  * a radix sort of the 3 nt (vertex, 3 k + l) pairs by vertex (hipCUB,
//    stable: fans in tria order; ~25 bits): latency-bound passes whose cost
//    does not grow with np.
// The sorts are chosen by size (r03, C2 / C3 steps).  With np > 5 * 3 nt (C3:
// 16.8 M vertices, 2.3 M pairs) the counting sort's memset and scan over np
// competed with the main stream's derived-data pass (step 2.11 -> 2.20 ms); at
// C2 (1.7 M vertices, 0.5 M pairs) the radix sort's passes were the surface
// stream's critical path (step 0.44 -> 0.36 ms with the counting sort).  A
// compacted-id counting sort (bitmap of the boundary vertices) lost both:
// 2.3 M atomicOr on 525 K words serialise.
#include "pmx_device.h"
#include "pmx_kernels.h"
#include "pmx_internal.h"
#include <algorithm>

__global__ __launch_bounds__(256) void k_nt_count(const TriRec *__restrict__ tris, int64_t nt,
                                                  unsigned *__restrict__ cnt) {
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nt;
       k += (int64_t)gridDim.x * blockDim.x) {
    const TriRec t = tris[k];
    if (t.v[0] <= 0) continue;
    for (int l = 0; l < 3; l++) atomicAdd(&cnt[t.v[l]], 1u);
  }
}
__global__ __launch_bounds__(256) void k_nt_fill(const TriRec *__restrict__ tris, int64_t nt,
                                                 const unsigned *__restrict__ off, unsigned *__restrict__ cnt,
                                                 int *__restrict__ list, int2 *__restrict__ range,
                                                 uint8_t *__restrict__ own) {
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nt;
       k += (int64_t)gridDim.x * blockDim.x) {
    const TriRec t = tris[k];
    for (int l = 0; l < 3; l++) {
      if (t.v[0] <= 0) { range[3 * k + l] = make_int2(0, 0); own[3 * k + l] = 0; continue; }
      const int v = t.v[l];
      const unsigned lo = off[v], hi = off[v + 1];
      const unsigned left = atomicSub(&cnt[v], 1u);          // hi - lo, ..., 1
      list[lo + left - 1] = (int)k;
      range[3 * k + l] = make_int2((int)lo, (int)hi);
      own[3 * k + l] = left == 1u ? 1 : 0;                   // exactly one writer per fan
    }
  }
}
__global__ __launch_bounds__(256) void k_nt_sort(int64_t nt, const int2 *__restrict__ range,
                                                 const uint8_t *__restrict__ own, int *__restrict__ list) {
  for (int64_t i = 3 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * (nt + 1);
       i += (int64_t)gridDim.x * blockDim.x) {
    if (!own[i]) continue;
    const int2 r = range[i];
    for (int a = r.x + 1; a < r.y; a++) {                 // insertion sort of the fan
      const int x = list[a];
      int b = a - 1;
      while (b >= r.x && list[b] > x) { list[b + 1] = list[b]; b--; }
      list[b + 1] = x;
    }
  }
}
__global__ __launch_bounds__(256) void k_nt_pairs(const TriRec *__restrict__ tris, int64_t nt,
                                                  unsigned *__restrict__ key, int *__restrict__ val) {
  for (int64_t k = 1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nt;
       k += (int64_t)gridDim.x * blockDim.x) {
    const TriRec t = tris[k];
    for (int l = 0; l < 3; l++) {
      key[3 * (k - 1) + l] = (unsigned)t.v[l];
      val[3 * (k - 1) + l] = (int)(3 * k + l);
    }
  }
}
__global__ __launch_bounds__(256) void k_nt_runs(const unsigned *__restrict__ key, const int *__restrict__ val,
                                                 int64_t m, int2 *__restrict__ range, int *__restrict__ list) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    list[i] = val[i] / 3;
    if (i > 0 && key[i - 1] == key[i]) continue;           // not the start of a run
    int64_t j = i + 1;
    while (j < m && key[j] == key[i]) j++;
    for (int64_t q = i; q < j; q++) range[val[q]] = make_int2((int)i, (int)j);
  }
}


// The fans by rotation (r05), for a closed manifold surface -- every
// boundary of a ParMmg group's volume mesh, interfaces included: each
// (tria, corner) slot walks its vertex's fan through the tria adjacency
// (Mmg's adjt: edge i opposite vertex i) and writes its tria into the window
// of the fan's owner (its smallest tria) at its rank: the fan's increasing
// tria order of PMMG_precompute_nodeTrias.  One kernel, no atomics, no
// np-sized arrays (the radix sort of C3's 2.3 M (vertex, tria) pairs took
// ~0.26 ms alone on the GPU).  A fan that meets an
// edge without a neighbour (open or non-manifold surface), a neighbour
// without the vertex, or more than FAN_CAP trias counts in *bad: the upload
// runs it once as a check, and a background with any such fan keeps the sort.
#define FAN_CAP 32
// one turn around v from tria k (corner l), the record of each tria in a
// register (one dependent load per step); f(tria, corner of v) per tria, k
// first; false if the fan does not close within FAN_CAP trias
__device__ __forceinline__ int sel3(const int a[3], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : a[2]; }
template <class F>
__device__ __forceinline__ bool fan_turn(const TriRec *__restrict__ tris, int k, int l, const TriRec &t0, F f) {
  const int v = sel3(t0.v, l);
  TriRec tc = t0;
  int cx = (l + 1) % 3, w = sel3(t0.v, (l + 2) % 3);
  f(k, l);
  for (int n = 1;; n++) {
    const int nxt = sel3(tc.nb, cx);               // across the edge {v, w}
    if (nxt == k) return true;                     // closed
    if (nxt <= 0 || n == FAN_CAP) return false;
    tc = tris[nxt];
    const int cv = tc.v[0] == v ? 0 : tc.v[1] == v ? 1 : tc.v[2] == v ? 2 : -1;
    const int cw = tc.v[0] == w ? 0 : tc.v[1] == w ? 1 : tc.v[2] == w ? 2 : -1;
    if (cv < 0 || cw < 0 || cv == cw || tc.v[0] <= 0) return false;
    f(nxt, cv);
    w = sel3(tc.v, 3 - cv - cw);                   // the other edge at v: {v, w'}
    cx = cw;
  }
}
// Every slot walks its fan once: the fan's window is its owner's (the
// smallest tria), and the slot's tria goes to the window at its rank in the
// fan (the number of smaller members) -- the sorted fan without a sort and no
// dependent chain beyond the walk itself.  r05 A/Bs at C3 (rocprof, beside
// the main stream): this 0.12 ms; an owner sorting its fan in global memory
// (a ~35-deep dependent chain) 0.19 ms; only the local minima walking and the
// owner sorting in LDS (2.3 M walks -> 0.8 M, but serial chains in few
// threads) 0.23 ms, step 2.061 vs 2.042 ms (profiles/r05_c3_sweep_fans_owner_lds.log).
// vown (the check only): each fan's owner slot writes its window base at
// its vertex; k_fan_check then finds the vertices whose slots belong to more
// than one fan (two surface sheets touching at a vertex: a group pinched
// there), which the rotation alone cannot see.  No per-vertex counts, no
// np-sized memset: every surface vertex has at least one fan owner, and no
// other vertex is read.  (r06 first version: a per-vertex tria count by
// atomics after an np-sized memset, 0.24 ms at C3 beside the step's prefix.)
__global__ __launch_bounds__(256) void k_fan_rotate(const TriRec *__restrict__ tris, int64_t nt,
                                                    int2 *__restrict__ range, int *__restrict__ list,
                                                    unsigned *__restrict__ bad, int *__restrict__ vown) {
  unsigned nbad = 0;
  for (int64_t i = 3 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * (nt + 1);
       i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / 3), l = (int)(i - 3 * (int64_t)k);
    const TriRec t0 = tris[k];
    if (t0.v[0] <= 0) { range[i] = make_int2(0, 0); continue; }
    int n = 0, rank = 0, own = k, lown = l;
    const bool ok = fan_turn(tris, k, l, t0, [&](int g, int c) {
      n++;
      rank += g < k ? 1 : 0;
      if (g < own) { own = g; lown = c; }
    });
    if (!ok) { nbad++; range[i] = make_int2(0, 0); continue; }
    const int base = (int)((3 * (int64_t)own + lown - 3) * FAN_CAP);
    range[i] = make_int2(base, base + n);
    list[base + rank] = k;
    if (vown && own == k && lown == l) vown[sel3(t0.v, l)] = base;
  }
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}
__global__ __launch_bounds__(256) void k_fan_check(const TriRec *__restrict__ tris, int64_t nt,
                                                   const int2 *__restrict__ range, const int *__restrict__ vown,
                                                   unsigned *__restrict__ bad) {
  unsigned nbad = 0;
  for (int64_t i = 3 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * (nt + 1);
       i += (int64_t)gridDim.x * blockDim.x) {
    const int2 r = range[i];
    if (r.y <= r.x) continue;                      // deleted tria (a failed fan is counted already)
    const int k = (int)(i / 3), l = (int)(i - 3 * (int64_t)k);
    const int v = tris[k].v[l];
    if (vown[v] != r.x) nbad++;
  }
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}

static unsigned fan_blocks(int64_t n, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
}

bool pmx_ctx::fan_rotation(hipStream_t s, unsigned *d_bad, bool check) {
  const pmx_call C{this, "node trias", s};
  const int64_t m = 3 * nt;
  if (!C.grow(d_ntrange, (size_t)(3 * (nt + 1))) || !C.grow(d_ntlist, (size_t)(m * FAN_CAP)))
    return false;
  if (check && !C.grow(d_ntkey, (size_t)(np + 2))) return false;
  int *vown = check ? reinterpret_cast<int *>(d_ntkey.p) : nullptr;
  const unsigned nb = fan_blocks(m, 16384);
  hipLaunchKernelGGL(k_fan_rotate, dim3(nb), dim3(256), 0, s, d_tris.p, nt, d_ntrange.p, d_ntlist.p, d_bad,
                     vown);
  if (check)
    hipLaunchKernelGGL(k_fan_check, dim3(nb), dim3(256), 0, s, d_tris.p, nt, (const int2 *)d_ntrange.p,
                       (const int *)vown, d_bad);
  return C.hip(hipGetLastError(), "launch");
}

// the upload's check: the fans of this background by rotation, their
// failures (open, non-manifold, pinched, over FAN_CAP) into
// h_nbad[PMX_H_BAD_FANS] (read after the upload's final sync).
// PMX_FAN_ROTATION=0 keeps the sort (A/B, tests).
bool pmx_ctx::check_fans(hipStream_t s) {
  const pmx_call C{this, "node trias", s};
  fan_rot = false;
  h_nbad.p[PMX_H_BAD_FANS] = 1u;
  if (nt < 1 || 3 * (nt + 1) * (int64_t)FAN_CAP > (int64_t)INT32_MAX) return true;   // int windows
  const char *e = getenv("PMX_FAN_ROTATION");
  if (e && e[0] == '0') return true;
  if (!C.grow(d_wfar, PMX_D_WORDS)) return false;
  // the vertices' fan owners (np-sized, no memset): a vertex where several
  // surface sheets touch has more than one fan
  if (!C.grow(d_ntkey, (size_t)(np + 2)) ||
      !C.grow(d_ntrange, (size_t)(3 * (nt + 1))) || !C.grow(d_ntlist, (size_t)(3 * nt * FAN_CAP))) {
    // no room for the check or the fan windows (32 per tria corner): the
    // surface keeps the sort-built fans, the upload goes on
    (void)hipGetLastError();
    err.clear();
    return true;
  }
  unsigned *bad = d_wfar.p + PMX_D_FANS_CHECK;
  return C.hip(hipMemsetAsync(bad, 0, sizeof(unsigned), s), "memset") && fan_rotation(s, bad, true) &&
         C.hip(hipMemcpyAsync(h_nbad.p + PMX_H_BAD_FANS, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s), "check");
}

// the counting sort over the vertex ids
static bool node_trias_counting(const pmx_call &C) {
  pmx_ctx *c = C.ctx;
  const int64_t m = 3 * c->nt, np = c->np, nt = c->nt;
  if (!C.grow(c->d_ntkey, (size_t)(2 * (np + 2))) || !C.grow(c->d_ntval, (size_t)(3 * (nt + 1))) ||
      !C.grow(c->d_ntrange, (size_t)(3 * (nt + 1))) || !C.grow(c->d_ntlist, (size_t)m))
    return false;
  unsigned *cnt = c->d_ntkey.p, *off = c->d_ntkey.p + (np + 2);
  uint8_t *own = reinterpret_cast<uint8_t *>(c->d_ntval.p);
  if (!C.hip(hipMemsetAsync(cnt, 0, (size_t)(np + 2) * sizeof(unsigned), C.s), "memset")) return false;
  const unsigned nb = fan_blocks(nt, 4096);
  hipLaunchKernelGGL(k_nt_count, dim3(nb), dim3(256), 0, C.s, c->d_tris.p, nt, cnt);
  if (!C.exclusive_sum(c->d_nttmp, cnt, off, np + 2, "scan")) return false;
  hipLaunchKernelGGL(k_nt_fill, dim3(nb), dim3(256), 0, C.s, c->d_tris.p, nt, (const unsigned *)off, cnt,
                     c->d_ntlist.p, c->d_ntrange.p, own);
  hipLaunchKernelGGL(k_nt_sort, dim3(fan_blocks(m, 4096)), dim3(256), 0, C.s, nt, (const int2 *)c->d_ntrange.p,
                     (const uint8_t *)own, c->d_ntlist.p);
  return C.hip(hipGetLastError(), "launch");
}

// the radix sort of the (vertex, 3 k + l) pairs
static bool node_trias_radix(const pmx_call &C) {
  pmx_ctx *c = C.ctx;
  const int64_t nt = c->nt, m = 3 * nt;
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) <= c->np) bits++;
  if (!C.grow(c->d_ntkey, (size_t)(2 * m)) || !C.grow(c->d_ntval, (size_t)(2 * m)) ||
      !C.grow(c->d_ntrange, (size_t)(3 * (nt + 1))) || !C.grow(c->d_ntlist, (size_t)m))
    return false;
  unsigned *key = c->d_ntkey.p;
  int *val = c->d_ntval.p;
  hipLaunchKernelGGL(k_nt_pairs, dim3(fan_blocks(nt, 4096)), dim3(256), 0, C.s, c->d_tris.p, nt, key, val);
  if (!C.sort_pairs(c->d_nttmp, (const unsigned *)key, key + m, (const int *)val, val + m, m, bits, "sort"))
    return false;
  hipLaunchKernelGGL(k_nt_runs, dim3(fan_blocks(m, 8192)), dim3(256), 0, C.s, (const unsigned *)key + m,
                     (const int *)val + m, m, c->d_ntrange.p, c->d_ntlist.p);
  return C.hip(hipGetLastError(), "launch");
}

bool pmx_ctx::build_node_trias(hipStream_t s, bool check) {
  const pmx_call C{this, "node trias", s};
  const int64_t m = 3 * nt;
  if (m < 1) return true;
  // check: the upload's check again (a FRESH step: what a new background
  // costs), the vertices' fan owners beside the rotation
  if (fan_rot) return fan_rotation(s, d_wfar.p + PMX_D_FANS_STEP, check);
  return np <= 5 * m ? node_trias_counting(C) : node_trias_radix(C);
}
