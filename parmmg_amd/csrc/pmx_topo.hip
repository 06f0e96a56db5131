// pmx_topo.hip -- background-mesh topology on gfx950.
//
// pmx_build_adja  <- MMG3D_hashTetra's face adjacency (Mmg; called by ParMmg
//                    at src/libparmmg1.c:272, src/distributemesh_pmmg.c:1185,
//                    src/metis_pmmg.c:756, ...): adja[4*(k-1)+1+f] = 4*k'+f'
// pmx_build_bdry  <- MMG5_chkBdryTria + MMG3D_hashTria on the old-group
//                    snapshot (src/grpsplit_pmmg.c:400-414): boundary trias
//                    of the faces without a neighbour, in (tet, face) order,
//                    vertices in MMG5_idir order, and their edge adjacency
//                    adjt[3*(k-1)+1+e] = 3*k'+e'
// pmx_bdry_device    its device part, on device arrays: pmx_build_bdry wraps
//                    it, an adopt with a surface calls it on the tet records
//
// Hash-free face matching: every face (edge) record goes to the bucket of its
// smallest vertex (count, exclusive scan, scatter); a face's partner is the
// record of the same bucket with the same two other vertices.  Buckets hold
// ~4 ne / np ~ 24 faces, the threads of one bucket are adjacent and read its
// records together.  The result does not depend on the order inside a bucket:
// an interior face of a valid mesh has exactly one partner (a face with more
// than one is non-manifold: reported, left 0, like the CPU builders of
// parmmg_amd/csrc/meshgen.c that the tests compare against).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>
#include "pmx_internal.h"


// MMG5_idir: local vertices of face f (opposite vertex f), outward order
__constant__ int TOPO_IDIR[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};

__device__ __forceinline__ void sort3i(int &a, int &b, int &c) {
  int t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
}

// ---- tet faces -------------------------------------------------------------------

// One thread per tet (its 4 faces), the faces of a workgroup aggregated per
// bucket (smallest vertex) in an LDS hash table: one global atomic per
// distinct bucket and workgroup instead of one per face (the neighbouring
// tets of a workgroup share most of their vertices; per-face atomics cost
// 3.7 ms of 4.4 at 10M tets).
#define FACE_HT 2048
__device__ __forceinline__ void face_key(const int4 t, int f, int &a, int &b, int &c) {
  const int v[4] = {t.x, t.y, t.z, t.w};
  a = v[TOPO_IDIR[f][0]];
  b = v[TOPO_IDIR[f][1]];
  c = v[TOPO_IDIR[f][2]];
  sort3i(a, b, c);
}
// slot of key a (inserted if absent); the table holds < FACE_HT / 2 keys
__device__ __forceinline__ int ht_slot(int *keys, int a) {
  unsigned h = ((unsigned)a * 2654435761u) >> (32 - 11);
  for (;;) {
    const int old = atomicCAS(&keys[h], -1, a);
    if (old == -1 || old == a) return (int)h;
    h = (h + 1) & (FACE_HT - 1);
  }
}

__global__ __launch_bounds__(256) void k_face_count(const int4 *__restrict__ tv, int64_t ne,
                                                    unsigned *__restrict__ cnt) {
  __shared__ int keys[FACE_HT];
  __shared__ unsigned cnts[FACE_HT];
  for (int i = threadIdx.x; i < FACE_HT; i += blockDim.x) { keys[i] = -1; cnts[i] = 0u; }
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (k <= ne) {
    const int4 t = tv[k];
    if (t.x > 0) {                               // !MG_EOK: no faces
      for (int f = 0; f < 4; f++) {
        int a, b, c;
        face_key(t, f, a, b, c);
        atomicAdd(&cnts[ht_slot(keys, a)], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FACE_HT; i += blockDim.x)
    if (keys[i] >= 0) atomicAdd(cnt + keys[i], cnts[i]);
}

__global__ __launch_bounds__(256) void k_face_scatter(const int4 *__restrict__ tv, int64_t ne,
                                                      unsigned *__restrict__ cursor,
                                                      int4 *__restrict__ rec) {
  __shared__ int keys[FACE_HT];
  __shared__ unsigned cnts[FACE_HT];
  for (int i = threadIdx.x; i < FACE_HT; i += blockDim.x) { keys[i] = -1; cnts[i] = 0u; }
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
  int4 t = make_int4(0, 0, 0, 0);
  int slot[4] = {0, 0, 0, 0};
  unsigned rank[4] = {0u, 0u, 0u, 0u};
  if (k <= ne) {
    t = tv[k];
    if (t.x > 0) {
      for (int f = 0; f < 4; f++) {
        int a, b, c;
        face_key(t, f, a, b, c);
        slot[f] = ht_slot(keys, a);
        rank[f] = atomicAdd(&cnts[slot[f]], 1u);   // place inside the workgroup's run
      }
    }
  }
  __syncthreads();
  // one reservation per bucket: the workgroup's run starts there
  for (int i = threadIdx.x; i < FACE_HT; i += blockDim.x)
    if (keys[i] >= 0) cnts[i] = atomicAdd(cursor + keys[i], cnts[i]);
  __syncthreads();
  if (k <= ne && t.x > 0) {
    for (int f = 0; f < 4; f++) {
      int a, b, c;
      face_key(t, f, a, b, c);
      rec[cnts[slot[f]] + rank[f]] = make_int4(a, b, c, (int)(4 * k + f));
    }
  }
}

// One thread per record: its partner in the bucket of its smallest vertex,
// with the records staged in LDS.  A workgroup owns MATCH_R consecutive
// records and loads them with MATCH_PAD records on either side (coalesced,
// 16 KB); a record whose bucket lies inside that window is compared against
// the LDS copy, any other (a bucket longer than the pads) against global
// memory: one global read per record and window instead of one per (record,
// bucket member), ~24 x 16 B per record.
#define MATCH_R 512
#define MATCH_PAD 256
__global__ __launch_bounds__(256) void k_face_match_lds(const int4 *__restrict__ rec, int64_t nb,
                                                        const unsigned *__restrict__ off,
                                                        int *__restrict__ adja,
                                                        unsigned *__restrict__ nbad) {
  __shared__ int4 win[MATCH_R + 2 * MATCH_PAD];
  const int64_t nrec = (int64_t)off[nb];
  const int64_t s0 = (int64_t)blockIdx.x * MATCH_R;
  const int64_t w0 = s0 - MATCH_PAD;              // window start (may be negative)
  for (int i = threadIdx.x; i < MATCH_R + 2 * MATCH_PAD; i += blockDim.x) {
    const int64_t r = w0 + i;
    win[i] = (r >= 0 && r < nrec) ? rec[r] : make_int4(-1, -1, -1, 0);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < MATCH_R; j += blockDim.x) {
    const int64_t s = s0 + j;
    if (s >= nrec) break;
    const int4 me = win[MATCH_PAD + j];
    const int64_t lo = off[me.x], hi = off[me.x + 1];
    int partner = 0, n = 0;
    if (lo >= w0 && hi <= w0 + MATCH_R + 2 * MATCH_PAD) {
      for (int64_t r = lo; r < hi; r++) {
        const int4 o = win[r - w0];
        if (r != s && o.y == me.y && o.z == me.z) { partner = o.w; n++; }
      }
    } else {
      for (int64_t r = lo; r < hi; r++) {
        const int4 o = rec[r];
        if (r != s && o.y == me.y && o.z == me.z) { partner = o.w; n++; }
      }
    }
    adja[me.w - 3] = (n == 1) ? partner : 0;
    if (n > 1) atomicAdd(nbad, 1u);
  }
}

static void launch_face_match(const int4 *rec, int64_t ne, int64_t np, const unsigned *off, int *dadja,
                              unsigned *nbad, hipStream_t s) {
  hipLaunchKernelGGL(k_face_match_lds, dim3((unsigned)std::max<int64_t>((4 * ne + MATCH_R - 1) / MATCH_R, 1)),
                     dim3(256), 0, s, rec, np + 1, off, dadja, nbad);
}

// ---- boundary trias and their edge adjacency -------------------------------------

// where a tet's face adjacency is read: entry (k, f) at p[stride * k + off + f],
// 0 = no neighbour.  Mmg's adja (4 ne + 5 ints): stride 4, off -3; the tet
// records' neighbour fields: stride 8, off 4
struct FaceAdj {
  const int *p;
  int stride, off;
  __device__ __forceinline__ int operator()(int64_t k, int f) const { return p[stride * k + off + f]; }
};

__global__ __launch_bounds__(256) void k_bdry_count(const int4 *__restrict__ tv, FaceAdj adja, int64_t ne,
                                                    unsigned *__restrict__ cnt) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (k > ne) return;
  unsigned c = 0;
  if (tv[k].x > 0) {                              // !MG_EOK tets have no faces
#pragma unroll
    for (int f = 0; f < 4; f++) c += adja(k, f) == 0 ? 1u : 0u;
  }
  cnt[k - 1] = c;
}

__global__ __launch_bounds__(256) void k_bdry_write(const int4 *__restrict__ tv, FaceAdj adja, int64_t ne,
                                                    const unsigned *__restrict__ pos,
                                                    int *__restrict__ tria) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (k > ne) return;
  const int4 t = tv[k];
  if (t.x <= 0) return;
  const int v[4] = {t.x, t.y, t.z, t.w};
  int64_t p = pos[k - 1] + 1;                    // 1-based tria index, (k, f) order
  for (int f = 0; f < 4; f++) {
    if (adja(k, f)) continue;
    tria[3 * p + 0] = v[TOPO_IDIR[f][0]];
    tria[3 * p + 1] = v[TOPO_IDIR[f][1]];
    tria[3 * p + 2] = v[TOPO_IDIR[f][2]];
    p++;
  }
}

// edge e of tria k joins its vertices (e+1)%3 and (e+2)%3
__global__ __launch_bounds__(256) void k_edge_count(const int *__restrict__ tria, int64_t nt,
                                                    unsigned *__restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // 3(k-1)+e
  if (i >= 3 * nt) return;
  const int64_t k = i / 3 + 1;
  const int e = (int)(i % 3);
  const int a = tria[3 * k + (e + 1) % 3], b = tria[3 * k + (e + 2) % 3];
  atomicAdd(cnt + min(a, b), 1u);
}

__global__ __launch_bounds__(256) void k_edge_scatter(const int *__restrict__ tria, int64_t nt,
                                                      unsigned *__restrict__ cursor,
                                                      int2 *__restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * nt) return;
  const int64_t k = i / 3 + 1;
  const int e = (int)(i % 3);
  const int a = tria[3 * k + (e + 1) % 3], b = tria[3 * k + (e + 2) % 3];
  const unsigned s = atomicAdd(cursor + min(a, b), 1u);
  rec[s] = make_int2(max(a, b), (int)(3 * k + e));
}

__global__ __launch_bounds__(256) void k_edge_match(const int2 *__restrict__ rec, int64_t nrec,
                                                    const unsigned *__restrict__ off,
                                                    const int *__restrict__ bucket_of,
                                                    int *__restrict__ adjt) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nrec) return;
  const int2 me = rec[s];
  const int a = bucket_of[s];
  const unsigned lo = off[a], hi = off[a + 1];
  int partner = 0, n = 0;
  for (unsigned r = lo; r < hi; r++) {
    const int2 o = rec[r];
    if (r != (unsigned)s && o.x == me.x) { partner = o.y; n++; }
  }
  adjt[me.y - 2] = (n == 1) ? partner : 0;       // 3*(k-1)+1+e = owner - 2
}

// bucket index of every record (the records of bucket a fill [off[a], off[a+1]))
__global__ __launch_bounds__(256) void k_bucket_of(const unsigned *__restrict__ off, int64_t nb,
                                                   int *__restrict__ bucket_of) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= nb) return;
  for (unsigned r = off[a]; r < off[a + 1]; r++) bucket_of[r] = (int)a;
}

// ---- host side ---------------------------------------------------------------------

namespace {

// call-local device memory of n elements (released when the call returns);
// nullptr on failure
template <class T> T *local(pmx_ctx *ctx, DevBuf<T> &b, size_t n) { return pmx_dgrow(ctx, b, n) ? b.p : nullptr; }

// strided host connectivity -> device int4 stream (1-based, slot 0 zero)
int4 *upload_tets(pmx_ctx *ctx, int64_t ne, int64_t np, const int *tetra_v, int64_t stride, DevBuf<int4> &buf) {
  std::vector<int4> h((size_t)(ne + 1));
  h[0] = make_int4(0, 0, 0, 0);
  const char *tc = (const char *)tetra_v;
  for (int64_t k = 1; k <= ne; k++) {
    const int *v = (const int *)(tc + k * stride);
    if (v[0] <= 0) { h[(size_t)k] = make_int4(0, 0, 0, 0); continue; }   // !MG_EOK
    for (int l = 0; l < 4; l++)
      if (v[l] < 1 || v[l] > np) {
        ctx->err = "topology: tet vertex index out of range";
        return nullptr;
      }
    h[(size_t)k] = make_int4(v[0], v[1], v[2], v[3]);
  }
  int4 *d = local(ctx, buf, h.size());
  if (!d) return nullptr;
  if (hipMemcpyAsync(d, h.data(), h.size() * sizeof(int4), hipMemcpyHostToDevice, ctx->stream) !=
      hipSuccess)
    return nullptr;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;
  return d;
}

// device adjacency from the device connectivity stream
bool build_adja_dev(const pmx_call &C, const int4 *tv, int64_t ne, int64_t np, int *dadja, unsigned *nbad_out) {
  pmx_ctx *ctx = C.ctx;
  hipStream_t s = C.s;
  DevBuf<unsigned> b_cnt, b_off, b_nbad;
  DevBuf<int4> b_rec;
  DevBuf<char> tmp;
  unsigned *cnt = local(ctx, b_cnt, (size_t)(np + 2));
  unsigned *off = local(ctx, b_off, (size_t)(np + 2));
  int4 *rec = local(ctx, b_rec, (size_t)(4 * ne));
  unsigned *nbad = local(ctx, b_nbad, 1);
  if (!cnt || !off || !rec || !nbad) return C.fail("hipMalloc");
  hipMemsetAsync(cnt, 0, sizeof(unsigned) * (size_t)(np + 2), s);
  hipMemsetAsync(nbad, 0, sizeof(unsigned), s);
  hipMemsetAsync(dadja, 0, sizeof(int) * (size_t)(4 * ne + 5), s);
  hipLaunchKernelGGL(k_face_count, dim3(pmx_call::blocks(ne)), dim3(256), 0, s, tv, ne, cnt);
  if (!C.exclusive_sum(tmp, (const unsigned *)cnt, off, np + 2, "scan")) return C.fail("scan");
  hipMemcpyAsync(cnt, off, sizeof(unsigned) * (size_t)(np + 2), hipMemcpyDeviceToDevice, s);
  hipLaunchKernelGGL(k_face_scatter, dim3(pmx_call::blocks(ne)), dim3(256), 0, s, tv, ne, cnt, rec);
  launch_face_match(rec, ne, np, off, dadja, nbad, s);
  if (hipMemcpyAsync(nbad_out, nbad, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return C.fail("launch");
  return true;
}

}  // namespace



// face adjacency of a device connectivity stream with the context's buffers
// (promoted backgrounds: the new tets are already on the device)
bool pmx_ctx_build_adja_device(pmx_ctx *ctx, const int4 *tv, int64_t ne, int64_t np, int *dadja,
                               hipStream_t s, unsigned *h_nbad) {
  const pmx_call C{ctx, "device adjacency", s};
  size_t bytes = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const unsigned *)nullptr, (unsigned *)nullptr,
                                   (int)(np + 2), s);
  if (!pmx_dgrow(ctx, ctx->d_tcnt, (size_t)(np + 2)) || !pmx_dgrow(ctx, ctx->d_toff, (size_t)(np + 2)) ||
      !pmx_dgrow(ctx, ctx->d_trec, (size_t)(4 * ne)) || !pmx_dgrow(ctx, ctx->d_tbad, 1) ||
      !pmx_dgrow(ctx, ctx->d_ttmp, bytes))
    return false;
  unsigned *cnt = ctx->d_tcnt.p, *off = ctx->d_toff.p, *nbad = ctx->d_tbad.p;
  bool okk = hipMemsetAsync(cnt, 0, sizeof(unsigned) * (size_t)(np + 2), s) == hipSuccess &&
             hipMemsetAsync(nbad, 0, sizeof(unsigned), s) == hipSuccess &&
             hipMemsetAsync(dadja, 0, sizeof(int) * (size_t)(4 * ne + 5), s) == hipSuccess;
  if (!okk) return C.fail("memset");
  hipLaunchKernelGGL(k_face_count, dim3(pmx_call::blocks(ne)), dim3(256), 0, s, tv, ne, cnt);
  if (hipcub::DeviceScan::ExclusiveSum(ctx->d_ttmp.p, bytes, cnt, off, (int)(np + 2), s) != hipSuccess)
    return C.fail("scan");
  hipMemcpyAsync(cnt, off, sizeof(unsigned) * (size_t)(np + 2), hipMemcpyDeviceToDevice, s);
  hipLaunchKernelGGL(k_face_scatter, dim3(pmx_call::blocks(ne)), dim3(256), 0, s, tv, ne, cnt, ctx->d_trec.p);
  launch_face_match(ctx->d_trec.p, ne, np, off, dadja, nbad, s);
  if (h_nbad) {
    if (hipMemcpyAsync(h_nbad, nbad, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess)
      return C.fail("launch");
    return true;
  }
  unsigned hb = 0;
  if (hipMemcpyAsync(&hb, nbad, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return C.fail("launch");
  if (hb) return C.fail("non-manifold tet faces");
  return true;
}

// MMG5_chkBdryTria + MMG3D_hashTria on device arrays (pmx_internal.h): count,
// scan, one control word down for nt, write, then the edges bucketed by their
// smaller vertex and matched.  Everything stays in B.
bool pmx_bdry_device(const pmx_call &C, const int4 *tv, const int *adj, int adj_stride, int adj_off, int64_t ne,
                     int64_t np, bool want_adjt, int64_t maxnt, BdryDev &B, int64_t *nt_out, hipEvent_t e0,
                     hipEvent_t e1) {
  pmx_ctx *ctx = C.ctx;
  hipStream_t s = C.s;
  const FaceAdj fa{adj, adj_stride, adj_off};
  unsigned *tcnt = local(ctx, B.tcnt, (size_t)(ne + 1));
  unsigned *tpos = local(ctx, B.tpos, (size_t)(ne + 1));
  if (!tcnt || !tpos) return C.fail("hipMalloc");
  hipMemsetAsync(tcnt, 0, sizeof(unsigned) * (size_t)(ne + 1), s);
  if (e0) hipEventRecord(e0, s);
  hipLaunchKernelGGL(k_bdry_count, dim3(pmx_call::blocks(ne)), dim3(256), 0, s, tv, fa, ne, tcnt);
  if (!C.exclusive_sum(B.tmp, (const unsigned *)tcnt, tpos, ne + 1, "scan")) return C.fail("scan");
  unsigned nt_u = 0;
  if (!C.read_words(&nt_u, (const unsigned *)(tpos + ne), 1, "boundary face count")) return false;
  const int64_t nt = nt_u;
  if (nt > maxnt) return C.fail("more boundary faces than maxnt");
  int *dtria = local(ctx, B.tria, (size_t)(3 * (nt + 1)));
  if (!dtria) return C.fail("hipMalloc");
  hipMemsetAsync(dtria, 0, sizeof(int) * 3, s);
  hipLaunchKernelGGL(k_bdry_write, dim3(pmx_call::blocks(ne)), dim3(256), 0, s, tv, fa, ne, tpos, dtria);
  if (want_adjt && nt > 0) {
    unsigned *cnt = local(ctx, B.cnt, (size_t)(np + 2));
    unsigned *off = local(ctx, B.off, (size_t)(np + 2));
    int2 *rec = local(ctx, B.rec, (size_t)(3 * nt));
    int *bof = local(ctx, B.bof, (size_t)(3 * nt));
    int *dadjt = local(ctx, B.adjt, (size_t)(3 * nt + 4));
    if (!cnt || !off || !rec || !bof || !dadjt) return C.fail("hipMalloc");
    hipMemsetAsync(cnt, 0, sizeof(unsigned) * (size_t)(np + 2), s);
    hipMemsetAsync(dadjt, 0, sizeof(int) * (size_t)(3 * nt + 4), s);
    hipLaunchKernelGGL(k_edge_count, dim3(pmx_call::blocks(3 * nt)), dim3(256), 0, s, dtria, nt, cnt);
    if (!C.exclusive_sum(B.tmp2, (const unsigned *)cnt, off, np + 2, "scan")) return C.fail("scan");
    hipMemcpyAsync(cnt, off, sizeof(unsigned) * (size_t)(np + 2), hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(k_edge_scatter, dim3(pmx_call::blocks(3 * nt)), dim3(256), 0, s, dtria, nt, cnt, rec);
    hipLaunchKernelGGL(k_bucket_of, dim3(pmx_call::blocks(np + 1)), dim3(256), 0, s, off, np + 1, bof);
    hipLaunchKernelGGL(k_edge_match, dim3(pmx_call::blocks(3 * nt)), dim3(256), 0, s, rec, 3 * nt, off, bof,
                       dadjt);
  }
  if (e1) hipEventRecord(e1, s);
  *nt_out = nt;
  return true;
}

extern "C" {

int pmx_build_adja(pmx_ctx *ctx, int64_t ne, int64_t np, const int *tetra_v, int64_t tetra_stride,
                   int *adja) {
  if (!ctx || !tetra_v || !adja || ne < 1 || np < 1 || 4 * ne >= (1LL << 31)) {
    if (ctx) ctx->err = "pmx_build_adja: bad arguments";
    return 0;
  }
  hipSetDevice(ctx->device);
  const pmx_call C{ctx, "pmx_build_adja", ctx->stream};
  DevBuf<int4> b_tv;
  DevBuf<int> b_adja;
  int4 *tv = upload_tets(ctx, ne, np, tetra_v, tetra_stride, b_tv);
  if (!tv) return 0;                             // pmx_last_error says why
  int *dadja = local(ctx, b_adja, (size_t)(4 * ne + 5));
  DevEvent e0, e1;
  e0.create();
  e1.create();
  hipEventRecord(e0, ctx->stream);
  unsigned nbad = 0;
  const bool ok = dadja && build_adja_dev(C, tv, ne, np, dadja, &nbad);
  hipEventRecord(e1, ctx->stream);
  hipEventSynchronize(e1);
  float ms = 0.f;
  hipEventElapsedTime(&ms, e0, e1);
  ctx->topo_ms = ms;
  if (!ok) return 0;
  if (hipMemcpy(adja, dadja, sizeof(int) * (size_t)(4 * ne + 5), hipMemcpyDeviceToHost) != hipSuccess)
    return C.fail("download");
  if (nbad) return C.fail("non-manifold tet faces (left 0)");
  return 1;
}

int64_t pmx_build_bdry(pmx_ctx *ctx, int64_t ne, int64_t np, const int *tetra_v,
                       int64_t tetra_stride, const int *adja, int *tria, int64_t maxnt, int *adjt) {
  if (!ctx || !tetra_v || !adja || !tria || ne < 1 || np < 1) {
    if (ctx) ctx->err = "pmx_build_bdry: bad arguments";
    return -1;
  }
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  const pmx_call C{ctx, "pmx_build_bdry", s};
  DevBuf<int4> b_tv;
  DevBuf<int> b_adja;
  BdryDev B;
  int4 *tv = upload_tets(ctx, ne, np, tetra_v, tetra_stride, b_tv);
  int *dadja = local(ctx, b_adja, (size_t)(4 * ne + 5));
  if (!tv || !dadja) return C.fail("hipMalloc"), -1;
  hipMemcpyAsync(dadja, adja, sizeof(int) * (size_t)(4 * ne + 5), hipMemcpyHostToDevice, s);
  DevEvent e0, e1;
  e0.create();
  e1.create();
  int64_t nt = 0;
  if (!pmx_bdry_device(C, tv, dadja, 4, -3, ne, np, adjt != nullptr, maxnt, B, &nt, e0, e1)) return -1;
  hipEventSynchronize(e1);
  float ms = 0.f;
  hipEventElapsedTime(&ms, e0, e1);
  ctx->topo_ms = ms;
  if (hipGetLastError() != hipSuccess) return C.fail("launch"), -1;
  if (hipMemcpy(tria, B.tria.p, sizeof(int) * (size_t)(3 * (nt + 1)), hipMemcpyDeviceToHost) != hipSuccess)
    return C.fail("download"), -1;
  if (adjt && nt > 0 &&
      hipMemcpy(adjt, B.adjt.p, sizeof(int) * (size_t)(3 * nt + 4), hipMemcpyDeviceToHost) != hipSuccess)
    return C.fail("download"), -1;
  return nt;
}

double pmx_topo_ms(pmx_ctx *ctx) { return ctx ? ctx->topo_ms : -1.0; }

}  // extern "C"
