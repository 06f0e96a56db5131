// pmx_moveifc.hip -- the interface displacement of the uploaded group on the device.
//
// pmx_moveifc_begin  <- PMMG_set_color_tetra, PMMG_mark_interfacePoints and the
//                       negrp / nemin of PMMG_part_moveInterfaces
//                       (src/moveinterfaces_pmmg.c:119-134, 1052-1090, 1337-1344)
// pmx_moveifc_get_colors / _set_colors
//                    <- the two ends of the node-communicator exchange (:1369-1376,
//                       :1406-1413); the exchange itself stays with the caller
// pmx_moveifc_layer  <- one wave of the advancing front (:1415-1438 over
//                       PMMG_mark_boulevolp :832-933 and PMMG_mark_sideFront :947-1038)
// pmx_moveifc_part   <- PMMG_part_getInterfaces (:1150-1212)
//
// Semantics: DESIGN.md section 4, "Interface displacement".  "b beats a" is
// weight(b) < weight(a), strictly, so every reduction of the reference's
// sequential loops is a running strict minimum in which the first met stays.
//
// Begin.  Per point, integer atomicMin over the tet slots 4 k + iloc gives the
// first slot and the best weight; a second pass the first slot of that
// weight.  tmp is the mark there, the point is front when the best weight is
// below the first slot's.
//
// Layer.  One lane per front point walks its ball in the reference's
// breadth-first order, which depends on the mesh and the point's slot s only.
// A slot 4 k + j belongs to one point, the vertex j of tet k, so the walk
// keeps its list in two slot arrays that no other lane touches: pos (the
// layer's stamp and the position in the ball) and next (the following slot).
// A tet then knows which of its vertices' balls reached it, and its mark
// history in the sequential loop is its mark at the layer's start followed by
// those vertices' colours in ascending point order, each applied when it
// beats the current one.  That gives the new marks (written to a second
// buffer), the recolourings and the per-group losses D.  When negrp - D >=
// nemin for every local group the sequential loop never blocked, and the layer
// is committed: every recolouring is an event on the tet's three other
// vertices, a non-front vertex takes the event of least (weight, point, ball
// position) if it beats its tmp -- two 64-bit atomicMin passes, (weight,
// point) then (position, slot) among the winners.  Otherwise nothing has been
// committed and one lane replays the reference's loop over the compacted
// front and the stored ball lists, at most `steps` ball tets per launch (its
// cursor lives in global memory and the host relaunches).  The side fronts run on the final marks,
// one lane per touched point over its stored list.
// No kernel here waits on another workgroup; every atomic is an integer min,
// max or add, so no result depends on arrival order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <unordered_map>
#include "pmx_device.h"
#include "pmx_internal.h"

namespace {

#define MI_LMAX 10240              // MMG3D_LMAX
#define MI_NELEM_MIN 6             // PMMG_REDISTR_NELEM_MIN
#define MI_POS_BITS 14             // a ball position is < MI_LMAX <= 2^14
#define MI_POS_MASK ((1 << MI_POS_BITS) - 1)
#define MI_MAX_LAYER ((1 << (31 - MI_POS_BITS)) - 1)
#define MI_SEQ_STEPS 65536
#define MI_NOKEY 0xffffffffffffffffull

// control words
enum {
  MI_DELETED = 0,   // a deleted tet
  MI_BADREC = 1,    // a vertex outside 1..np, a neighbour outside 0..ne, or one that does not hold the point
  MI_BADGRP = 2,    // tet_group outside 0..nold_grp-1
  MI_BADW = 3,      // a colour that occurs with weight <= 0
  MI_NFRONT = 4,    // front points (begin: flagged; layer: walked)
  MI_OVF = 5,       // the smallest point whose ball overflowed (0xffffffff: none)
  MI_MAXBALL = 6,
  MI_NREC = 7,      // recolourings
  MI_TOUCHED = 8,
  MI_NEXT = 9,
  MI_SEQ_IP = 10,   // the sequential path's cursor into the front list
  MI_BLOCKS = 11,
  MI_NLIST = 12,    // entries of the front list
  MI_NCTL = 16
};

struct MiMap {
  const int *w;     // weight by colour, 0: no such colour
  int ncol, nprocs, myrank;
};

__device__ __forceinline__ unsigned mi_w(const MiMap &m, int c) { return (unsigned)m.w[c]; }
__device__ __forceinline__ int mi_nxt(int i) { return (i + 1) & 3; }   // MMG5_inxt3

// marks from the old groups; the refusals of begin
__global__ __launch_bounds__(256) void k_mi_color(const TetRec *__restrict__ tets, int64_t ne, int64_t np,
                                                  const int *__restrict__ tgrp, int nold, MiMap m,
                                                  int *__restrict__ mark, unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne) return;
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  const int4 v = recs[2 * k], nb = recs[2 * k + 1];
  const int n = (int)ne, P = (int)np;
  if (v.x <= 0) ctl[MI_DELETED] = 1u;
  if (v.x > P || v.y <= 0 || v.y > P || v.z <= 0 || v.z > P || v.w <= 0 || v.w > P || nb.x < 0 || nb.x > n ||
      nb.y < 0 || nb.y > n || nb.z < 0 || nb.z > n || nb.w < 0 || nb.w > n)
    ctl[MI_BADREC] = 1u;
  const int g = tgrp[k - 1];
  if (g < 0 || g >= nold) {
    ctl[MI_BADGRP] = 1u;
    mark[k] = 0;
    return;
  }
  const int c = m.nprocs * g + m.myrank;
  if (c >= m.ncol || m.w[c] <= 0) ctl[MI_BADW] = 1u;
  mark[k] = c;
}

// pass 0: first[p] = the first slot of p, wbest[p] = the best weight around p;
// pass 1: sbest[p] = the first slot of that weight
__global__ __launch_bounds__(256) void k_mi_begin_slots(const TetRec *__restrict__ tets, int64_t ne,
                                                        const int *__restrict__ mark, MiMap m, int pass,
                                                        unsigned *first, unsigned *wbest, unsigned *sbest) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne) return;
  const int4 v4 = reinterpret_cast<const int4 *>(tets)[2 * k];
  const int v[4] = {v4.x, v4.y, v4.z, v4.w};
  const unsigned w = mi_w(m, mark[k]);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const unsigned slot = (unsigned)(4 * k + j);
    if (pass == 0) {
      atomicMin(&first[v[j]], slot);
      atomicMin(&wbest[v[j]], w);
    } else if (wbest[v[j]] == w)
      atomicMin(&sbest[v[j]], slot);
  }
}

__global__ __launch_bounds__(256) void k_mi_begin_points(int64_t np, const int *__restrict__ mark, MiMap m,
                                                         const unsigned *__restrict__ first,
                                                         const unsigned *__restrict__ wbest,
                                                         const unsigned *__restrict__ sbest, int *__restrict__ tmp,
                                                         int *__restrict__ s, int *__restrict__ flag,
                                                         unsigned *__restrict__ ctl) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > np) return;
  const unsigned f = first[p];
  if (p == 0 || f == 0xffffffffu) {       // a point in no tet
    tmp[p] = -1;
    s[p] = -1;
    flag[p] = 0;
    return;
  }
  const unsigned sb = sbest[p];
  const bool front = wbest[p] < mi_w(m, mark[f >> 2]);
  tmp[p] = mark[sb >> 2];
  s[p] = (int)sb;
  flag[p] = front;
  if (front) atomicAdd(&ctl[MI_NFRONT], 1u);
}

// the ball of every front point p from its slot s[p], breadth-first through
// the three faces that hold p in the order inxt3: pos[slot] = stamp | position,
// next[slot] = the following slot (0 ends the list).  More than MI_LMAX - 2
// tets: the point is reported and its list left unfinished.
__global__ __launch_bounds__(64) void k_mi_walk(const TetRec *__restrict__ tets, int64_t np,
                                                const int *__restrict__ s, const int *__restrict__ flag, int *pos,
                                                int *next, int stamp, unsigned *__restrict__ ctl) {
  const int64_t p64 = (int64_t)blockIdx.x * 64 + threadIdx.x + 1;
  if (p64 > np) return;
  const int p = (int)p64;
  if (flag[p] == 0 || s[p] < 0) return;
  atomicAdd(&ctl[MI_NFRONT], 1u);
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  int cur = s[p], tail = cur, ilist = 1;
  pos[cur] = stamp;
  next[cur] = 0;
  while (cur) {
    const int k = cur >> 2;
    int i = cur & 3;
    const int4 nb4 = recs[2 * (int64_t)k + 1];
    const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
    for (int l = 0; l < 3; l++) {
      i = mi_nxt(i);
      const int k1 = nb[i];
      if (!k1) continue;
      const int4 v1 = recs[2 * (int64_t)k1];
      const int j1 = v1.x == p ? 0 : v1.y == p ? 1 : v1.z == p ? 2 : v1.w == p ? 3 : -1;
      if (j1 < 0) {
        ctl[MI_BADREC] = 1u;
        continue;
      }
      const int slot = 4 * k1 + j1;
      if ((pos[slot] & ~MI_POS_MASK) == stamp) continue;
      if (ilist > MI_LMAX - 3) {
        atomicMin(&ctl[MI_OVF], (unsigned)p);
        return;
      }
      pos[slot] = stamp | ilist;
      next[slot] = 0;
      next[tail] = slot;
      tail = slot;
      ilist++;
    }
    cur = next[cur];
  }
  atomicMax(&ctl[MI_MAXBALL], (unsigned)ilist);
}

// A tet's mark history: its mark, then the colours of the front vertices
// whose ball reached it, in ascending point order, each applied when it beats
// the current one.  pass 0: the final mark into newmark, the recolourings, the
// losses D[g] of the local groups and, per other vertex of a recoloured tet,
// key1 = min (weight, point).  pass 1: key2 = min (ball position, the vertex's
// slot) among the events that won key1.
__global__ __launch_bounds__(256) void k_mi_tets(const TetRec *__restrict__ tets, int64_t ne,
                                                 const int *__restrict__ mark, const int *__restrict__ tmp,
                                                 const int *__restrict__ pos, int stamp, MiMap m, int pass,
                                                 int *__restrict__ newmark, unsigned *D, unsigned long long *key1,
                                                 unsigned long long *key2, unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne) return;
  const int4 p4 = reinterpret_cast<const int4 *>(pos)[k];
  const int ps[4] = {p4.x, p4.y, p4.z, p4.w};
  int cur = mark[k];
  int nj = 0, jj[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    if ((ps[j] & ~MI_POS_MASK) == stamp) jj[nj++] = j;
  if (nj == 0) {
    if (pass == 0) newmark[k] = cur;
    return;
  }
  const int4 v4 = reinterpret_cast<const int4 *>(tets)[2 * k];
  const int v[4] = {v4.x, v4.y, v4.z, v4.w};
  // the reached vertices by ascending point
  for (int a = 1; a < nj; a++)
    for (int b = a; b > 0 && v[jj[b]] < v[jj[b - 1]]; b--) {
      const int t = jj[b];
      jj[b] = jj[b - 1];
      jj[b - 1] = t;
    }
  unsigned nrec = 0;
  for (int a = 0; a < nj; a++) {
    const int j = jj[a], ip = v[j], c = tmp[ip];
    const unsigned w = mi_w(m, c);
    if (!(w < mi_w(m, cur))) continue;
    const unsigned long long k1 = ((unsigned long long)w << 32) | (unsigned)ip;
    if (pass == 0) {
      nrec++;
      if (cur % m.nprocs == m.myrank) atomicAdd(&D[cur / m.nprocs], 1u);
    }
    int j2 = j;
    for (int t = 0; t < 3; t++) {
      j2 = mi_nxt(j2);
      const int q = v[j2];
      if (pass == 0) atomicMin(&key1[q], k1);
      else if (key1[q] == k1)
        atomicMin(&key2[q], ((unsigned long long)(ps[j] & MI_POS_MASK) << 32) | (unsigned)(4 * k + j2));
    }
    cur = c;
  }
  if (pass == 0) {
    newmark[k] = cur;
    if (nrec) atomicAdd(&ctl[MI_NREC], nrec);
  }
}

// the events on the points: a front point with one becomes touched (2), any
// other point next (3) and takes the winning event when it beats its tmp
__global__ __launch_bounds__(256) void k_mi_points(int64_t np, MiMap m, const unsigned long long *__restrict__ key1,
                                                   const unsigned long long *__restrict__ key2, int *tmp,
                                                   int *__restrict__ s, int *__restrict__ flag) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (p > np) return;
  const unsigned long long k1 = key1[p];
  if (k1 == MI_NOKEY) return;
  if (flag[p] != 0) {
    flag[p] = 2;
    return;
  }
  flag[p] = 3;
  const unsigned w = (unsigned)(k1 >> 32);
  if (w < mi_w(m, tmp[p])) {
    tmp[p] = tmp[(unsigned)k1];          // a front point's colour: no lane writes it here
    s[p] = (int)(unsigned)key2[p];
  }
}

// The reference's loop over the front points on the stored ball lists, one
// lane.  front: the points that were front at the layer's start, ascending
// (ctl[MI_NLIST] of them), from the cursor ctl[MI_SEQ_IP]; a launch ends after
// `steps` steps, a step being a ball tet visited or a listed point without a
// ball.  grp: negrp (nold entries), then nemin.
__global__ __launch_bounds__(64) void k_mi_seq(const TetRec *__restrict__ tets, const int *__restrict__ front,
                                               int *mark, int *tmp, int *s, int *flag, const int *__restrict__ next,
                                               MiMap m, int *grp, int nold, int steps, unsigned *ctl) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int *negrp = grp;
  const int *nemin = grp + nold;
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  const unsigned n = ctl[MI_NLIST];
  unsigned i = ctl[MI_SEQ_IP];
  unsigned nrec = 0, nblocks = 0, maxball = 0;
  int done = 0;
  for (; i < n && done < steps; i++) {
    const int ip = front[i];
    if (s[ip] < 0) {
      done++;
      continue;
    }
    const int color = tmp[ip];
    const unsigned wc = mi_w(m, color);
    int slot = s[ip];
    unsigned idx = 0;
    bool blocked = false;
    while (slot) {
      const int k = slot >> 2, j1 = slot & 3, old = mark[k];
      done++;
      if (wc < mi_w(m, old)) {
        if (old % m.nprocs == m.myrank) {
          const int g = old / m.nprocs;
          if (idx == 0 ? negrp[g] <= nemin[g] : negrp[g] == nemin[g]) {
            blocked = true;
            break;
          }
          negrp[g]--;
        }
        mark[k] = color;
        nrec++;
        const int4 v4 = recs[2 * (int64_t)k];
        const int v[4] = {v4.x, v4.y, v4.z, v4.w};
        int j2 = j1;
        for (int t = 0; t < 3; t++) {
          j2 = mi_nxt(j2);
          const int q = v[j2], fq = flag[q];
          if (fq != 1 && fq != 2) {
            if (wc < mi_w(m, tmp[q])) {
              tmp[q] = color;
              s[q] = 4 * k + j2;
            }
            flag[q] = 3;
          } else
            flag[q] = 2;
        }
      }
      idx++;
      slot = next[slot];
    }
    if (blocked) nblocks++;
    else if (idx > maxball) maxball = idx;
  }
  ctl[MI_SEQ_IP] = i;
  ctl[MI_NREC] += nrec;
  ctl[MI_BLOCKS] += nblocks;
  if (maxball > ctl[MI_MAXBALL]) ctl[MI_MAXBALL] = maxball;
}

// PMMG_mark_sideFront on the final marks: a touched point takes the lightest
// mark of its ball, the first in list order, and s moves there; then the next
// front: touched and next points
__global__ __launch_bounds__(64) void k_mi_side(int64_t np, const int *__restrict__ mark, MiMap m,
                                                const int *__restrict__ next, int *__restrict__ tmp,
                                                int *__restrict__ s, int *__restrict__ flag,
                                                unsigned *__restrict__ ctl) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x + 1;
  if (p > np) return;
  const int f = flag[p];
  if (f == 2) {
    int c = tmp[p], best = s[p];
    unsigned w = mi_w(m, c), len = 0;
    for (int slot = best; slot; slot = next[slot]) {
      const int mk = mark[slot >> 2];
      const unsigned wk = mi_w(m, mk);
      if (wk < w) {
        w = wk;
        c = mk;
        best = slot;
      }
      len++;
    }
    tmp[p] = c;
    s[p] = best;
    atomicAdd(&ctl[MI_TOUCHED], 1u);
    atomicMax(&ctl[MI_MAXBALL], len);
  }
  flag[p] = f >= 2;
  if (f >= 2) atomicAdd(&ctl[MI_NEXT], 1u);
}

__global__ __launch_bounds__(256) void k_mi_gather(int64_t n, const int *__restrict__ ip, const int *__restrict__ tmp,
                                                   int *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = tmp[ip[i]];
}

// every listed point (each once) takes its colour and joins the front
__global__ __launch_bounds__(256) void k_mi_scatter(int64_t n, const int *__restrict__ ip,
                                                    const int *__restrict__ color, int *__restrict__ tmp,
                                                    int *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tmp[ip[i]] = color[i];
  flag[ip[i]] = 1;
}

}  // namespace

// The displacement's state, valid for the background it began on
struct pmx_moveifc_state {
  int64_t ne = 0, np = 0;
  int nprocs = 1, myrank = 0, nold = 0, layer = 0;
  std::vector<int> displs, wcol, negrp, nemin;   // wcol: weight by colour, 0 = no such colour
  DevBuf<int> d_wcol, mark, mark2, tmp, s, flag, pos, next, grp, io, front;
  DevBuf<char> cub;
  DevBuf<unsigned> D, ctl, first;
  DevBuf<unsigned long long> key1, key2;
  DevEvent ev[2];
  MiMap map() const { return MiMap{d_wcol.p, (int)wcol.size(), nprocs, myrank}; }
};

namespace {

struct MoveIfc : pmx_call {
  pmx_moveifc_state *st;
  MoveIfc(pmx_ctx *c, const char *w) : pmx_call{c, w, c->stream}, st(c->moveifc) {}
  // the state of a begin on the current background
  bool live() {
    if (!st || !ctx->moveifc_valid || !ctx->have_bg) return fail("no displacement: call pmx_moveifc_begin");
    return true;
  }
  bool read_ctl(unsigned *h) { return read_words(h, (const unsigned *)st->ctl.p, MI_NCTL); }
  bool zero_ctl() {
    unsigned h[MI_NCTL] = {0};
    h[MI_OVF] = 0xffffffffu;
    return ok(hipMemcpyAsync(st->ctl.p, h, sizeof h, hipMemcpyHostToDevice, s), "control words") &&
           ok(hipStreamSynchronize(s), "control words");
  }
  bool elapsed(double &ms) {
    float t = 0.f;
    if (!ok(hipEventRecord(st->ev[1], s), "event record") || !sync("kernels") ||
        !ok(hipEventElapsedTime(&t, st->ev[0], st->ev[1]), "event time"))
      return false;
    ms = t;
    return true;
  }
  template <class T> bool down(T *dst, const T *src, int64_t n) {
    return !dst || n == 0 || ok(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, s), "download");
  }
};

}  // namespace

void pmx_moveifc_free(pmx_ctx *ctx) {
  pmx_moveifc_state *S = ctx->moveifc;   // its members release themselves
  ctx->moveifc = nullptr;
  ctx->moveifc_valid = false;
  ctx->moveifc_begin_ms = ctx->moveifc_layer_ms = -1.0;
  ctx->moveifc_fixed = false;
  ctx->moveifc_fix_ms = -1.0;
  delete S;
}

bool pmx_moveifc_live_marks(pmx_ctx *ctx, MoveIfcMarks *m) {
  const pmx_moveifc_state *S = ctx->moveifc;
  if (!S || !ctx->moveifc_valid || !ctx->have_bg) return false;
  *m = MoveIfcMarks{S->mark.p, S->ne, S->nprocs, S->myrank, S->nold, S->displs.data()};
  return true;
}

double pmx_moveifc_kernel_ms(pmx_ctx *ctx, int which) {
  if (!ctx->moveifc_valid) return -1.0;   // dropped by an upload, a promotion or an adoption
  return which == 19 ? ctx->moveifc_begin_ms : ctx->moveifc_layer_ms;
}

extern "C" {

int pmx_moveifc_begin(pmx_ctx *ctx, const int32_t *tet_group, const pmx_moveifc_map *map, int64_t *nfront) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_begin"};
  if (!ctx->have_bg) { L.fail("upload a group first"); return 0; }
  if (4 * ctx->ne >= (1LL << 31)) { L.fail("4 ne >= 2^31 (32-bit slots)"); return 0; }
  if (!map || !map->displsgrp || !map->mapgrp) { L.fail("map is NULL"); return 0; }
  const int nprocs = map->nprocs, myrank = map->myrank, nold = map->nold_grp;
  if (nprocs < 1 || myrank < 0 || myrank >= nprocs || nold < 1) {
    L.fail("nprocs < 1, myrank outside 0..nprocs-1 or nold_grp < 1");
    return 0;
  }
  int maxg = 0;
  if (map->displsgrp[0] != 0) { L.fail("displsgrp[0] != 0"); return 0; }
  for (int i = 0; i < nprocs; i++) {
    const int64_t n = (int64_t)map->displsgrp[i + 1] - map->displsgrp[i];
    if (n < 0) { L.fail("displsgrp decreases"); return 0; }
    maxg = (int)std::max<int64_t>(maxg, n);
  }
  if (map->displsgrp[myrank + 1] - map->displsgrp[myrank] != nold) {
    L.fail("displsgrp gives this rank another group count than nold_grp");
    return 0;
  }
  if ((int64_t)maxg * nprocs >= (1LL << 31)) { L.fail("colours >= 2^31"); return 0; }
  const int64_t ne = ctx->ne, np = ctx->np;
  const int *d_tgrp = nullptr;
  if (!tet_group) {
    int64_t pne = 0;
    if (!pmx_merge_tet_group(ctx, &d_tgrp, &pne)) { L.fail("tet_group is NULL and no merge plan is live"); return 0; }
    if (pne != ne) { L.fail("the merge plan's group is not the uploaded one (adopt it)"); return 0; }
  }
  hipStreamSynchronize(L.s);
  pmx_moveifc_free(ctx);
  pmx_moveifc_state *S = new pmx_moveifc_state();
  ctx->moveifc = S;
  L.st = S;
  auto no = [&](const char *what) {
    if (what) L.fail(what);
    pmx_moveifc_free(ctx);
    return 0;
  };
  S->ne = ne;
  S->np = np;
  S->nprocs = nprocs;
  S->myrank = myrank;
  S->nold = nold;
  S->displs.assign(map->displsgrp, map->displsgrp + nprocs + 1);
  S->wcol.assign((size_t)std::max(maxg, 1) * nprocs, 0);
  for (int r = 0; r < nprocs; r++)
    for (int g = 0; g < S->displs[r + 1] - S->displs[r]; g++) {
      const int w = map->mapgrp[S->displs[r] + g];
      S->wcol[(size_t)nprocs * g + r] = w > 0 ? w : 0;
    }
  S->negrp.resize(nold);
  S->nemin.resize(nold);
  for (int g = 0; g < nold; g++) {
    S->negrp[g] = map->mapgrp[S->displs[myrank] + g];
    S->nemin[g] = std::min(MI_NELEM_MIN, S->negrp[g] / 2 + 1);
  }
  const size_t nt = (size_t)(ne + 1), npt = (size_t)(np + 1);
  if (!L.grow(S->d_wcol, S->wcol.size()) || !L.grow(S->mark, nt) || !L.grow(S->mark2, nt) || !L.grow(S->tmp, npt) ||
      !L.grow(S->s, npt) || !L.grow(S->flag, npt) || !L.grow(S->pos, 4 * nt) || !L.grow(S->next, 4 * nt) ||
      !L.grow(S->grp, 2 * (size_t)nold) || !L.grow(S->D, (size_t)nold) || !L.grow(S->ctl, MI_NCTL) ||
      !L.grow(S->first, 3 * npt) || !L.grow(S->key1, npt) || !L.grow(S->key2, npt) ||
      (tet_group && !L.grow(S->io, (size_t)std::max<int64_t>(ne, 1))))
    return no(nullptr);
  if (!pmx_create_events(S->ev)) return no("event");
  hipStream_t s = L.s;
  if (!L.ok(hipEventRecord(S->ev[0], s), "event record")) return no(nullptr);
  if (!L.zero_ctl()) return no(nullptr);
  if (!L.ok(hipMemcpyAsync(S->d_wcol.p, S->wcol.data(), sizeof(int) * S->wcol.size(), hipMemcpyHostToDevice, s),
            "weights upload") ||
      (tet_group && ne > 0 &&
       !L.ok(hipMemcpyAsync(S->io.p, tet_group, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, s),
             "tet_group upload")) ||
      !L.ok(hipMemsetAsync(S->mark.p, 0, sizeof(int) * nt, s), "memset") ||
      !L.ok(hipMemsetAsync(S->pos.p, 0, sizeof(int) * 4 * nt, s), "memset") ||
      !L.ok(hipMemsetAsync(S->next.p, 0, sizeof(int) * 4 * nt, s), "memset") ||
      !L.ok(hipMemsetAsync(S->first.p, 0xff, sizeof(unsigned) * 3 * npt, s), "memset"))
    return no(nullptr);
  const MiMap m = S->map();
  const TetRec *tets = ctx->d_tets.p;
  const unsigned nbt = L.blocks(ne), nbp = L.blocks(np + 1);
  unsigned h[MI_NCTL];
  if (ne > 0)
    hipLaunchKernelGGL(k_mi_color, dim3(nbt), dim3(256), 0, s, tets, ne, np, tet_group ? (const int *)S->io.p : d_tgrp,
                       nold, m, S->mark.p, S->ctl.p);
  if (!L.read_ctl(h)) return no(nullptr);
  if (hipGetLastError() != hipSuccess) return no("colour launch");
  if (h[MI_DELETED]) return no("a deleted tet (v[0] <= 0): the reference wants a packed mesh");
  if (h[MI_BADREC]) return no("a tet record with a vertex outside 1..np or a neighbour outside 0..ne");
  if (h[MI_BADGRP]) return no("tet_group outside 0..nold_grp-1");
  if (h[MI_BADW]) return no("a colour that occurs has mapgrp <= 0");
  unsigned *first = S->first.p, *wbest = first + npt, *sbest = wbest + npt;
  if (ne > 0) {
    hipLaunchKernelGGL(k_mi_begin_slots, dim3(nbt), dim3(256), 0, s, tets, ne, (const int *)S->mark.p, m, 0, first,
                       wbest, sbest);
    hipLaunchKernelGGL(k_mi_begin_slots, dim3(nbt), dim3(256), 0, s, tets, ne, (const int *)S->mark.p, m, 1, first,
                       wbest, sbest);
  }
  hipLaunchKernelGGL(k_mi_begin_points, dim3(nbp), dim3(256), 0, s, np, (const int *)S->mark.p, m,
                     (const unsigned *)first, (const unsigned *)wbest, (const unsigned *)sbest, S->tmp.p, S->s.p,
                     S->flag.p, S->ctl.p);
  double ms = -1.0;
  if (!L.read_ctl(h) || !L.elapsed(ms)) return no(nullptr);
  ctx->moveifc_valid = true;
  ctx->moveifc_begin_ms = ms;
  if (nfront) *nfront = h[MI_NFRONT];
  return 1;
}

int pmx_moveifc_get_colors(pmx_ctx *ctx, int64_t n, const int *ip, int *color) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_get_colors"};
  if (!L.live()) return 0;
  pmx_moveifc_state &S = *L.st;
  if (n < 0 || (n > 0 && (!ip || !color))) { L.fail("n < 0 or a NULL array"); return 0; }
  for (int64_t i = 0; i < n; i++)
    if (ip[i] < 1 || ip[i] > S.np) { L.fail("a point outside 1..np"); return 0; }
  if (n == 0) return 1;
  if (!L.grow(S.io, 2 * (size_t)n)) return 0;
  std::vector<int> out((size_t)n);
  PMX_CK(L, hipMemcpyAsync(S.io.p, ip, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, L.s));
  hipLaunchKernelGGL(k_mi_gather, dim3(L.blocks(n)), dim3(256), 0, L.s, n, (const int *)S.io.p, (const int *)S.tmp.p,
                     S.io.p + n);
  if (!L.down(out.data(), (const int *)S.io.p + n, n) || !L.sync("gather")) return 0;
  std::copy(out.begin(), out.end(), color);
  return 1;
}

int pmx_moveifc_set_colors(pmx_ctx *ctx, int64_t n, const int *ip, const int *color) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_set_colors"};
  if (!L.live()) return 0;
  pmx_moveifc_state &S = *L.st;
  if (n < 0 || (n > 0 && (!ip || !color))) { L.fail("n < 0 or a NULL array"); return 0; }
  // a point listed twice keeps its last colour, as the reference's loop does
  std::unordered_map<int, int> last;
  for (int64_t i = 0; i < n; i++) {
    if (ip[i] < 1 || ip[i] > S.np) { L.fail("a point outside 1..np"); return 0; }
    if (color[i] < 0 || color[i] >= (int)S.wcol.size() || S.wcol[color[i]] <= 0) {
      L.fail("a colour of no group, or of one with mapgrp <= 0");
      return 0;
    }
    last[ip[i]] = color[i];
  }
  ctx->moveifc_fixed = false;           // the next layer moves the marks again
  if (n == 0) return 1;
  const int64_t u = (int64_t)last.size();
  std::vector<int> buf;
  buf.reserve(2 * (size_t)u);
  for (const auto &e : last) buf.push_back(e.first);
  for (int64_t i = 0; i < u; i++) buf.push_back(last[buf[(size_t)i]]);
  if (!L.grow(S.io, 2 * (size_t)u)) return 0;
  PMX_CK(L, hipMemcpyAsync(S.io.p, buf.data(), sizeof(int) * 2 * (size_t)u, hipMemcpyHostToDevice, L.s));
  hipLaunchKernelGGL(k_mi_scatter, dim3(L.blocks(u)), dim3(256), 0, L.s, u, (const int *)S.io.p,
                     (const int *)S.io.p + u, S.tmp.p, S.flag.p);
  return L.sync("scatter") ? 1 : 0;
}

int pmx_moveifc_layer(pmx_ctx *ctx, int64_t seq_steps, pmx_moveifc_stats *stats) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_layer"};
  if (!L.live()) return 0;
  pmx_moveifc_state &S = *L.st;
  if (seq_steps < 0) { L.fail("seq_steps < 0"); return 0; }
  const int steps = (int)std::min<int64_t>(seq_steps ? seq_steps : MI_SEQ_STEPS, 1 << 30);
  hipStream_t s = L.s;
  const int64_t ne = S.ne, np = S.np;
  const size_t nt = (size_t)(ne + 1), npt = (size_t)(np + 1);
  const int nold = S.nold;
  ctx->moveifc_layer_ms = -1.0;
  ctx->moveifc_fixed = false;
  if (S.layer >= MI_MAX_LAYER) {          // the stamps start again
    PMX_CK(L, hipMemsetAsync(S.pos.p, 0, sizeof(int) * 4 * nt, s));
    S.layer = 0;
  }
  const int stamp = ++S.layer << MI_POS_BITS;
  const MiMap m = S.map();
  const TetRec *tets = ctx->d_tets.p;
  const unsigned nbt = L.blocks(ne), nbp = L.blocks(np), nbw = (unsigned)std::max<int64_t>((np + 63) / 64, 1);
  unsigned h[MI_NCTL];
  pmx_moveifc_stats T{};
  PMX_CK(L, hipEventRecord(S.ev[0], s));
  if (!L.zero_ctl()) return 0;
  PMX_CK(L, hipMemsetAsync(S.D.p, 0, sizeof(unsigned) * (size_t)nold, s));
  PMX_CK(L, hipMemsetAsync(S.key1.p, 0xff, sizeof(unsigned long long) * npt, s));
  PMX_CK(L, hipMemsetAsync(S.key2.p, 0xff, sizeof(unsigned long long) * npt, s));
  // 1. the balls
  hipLaunchKernelGGL(k_mi_walk, dim3(nbw), dim3(64), 0, s, tets, np, (const int *)S.s.p, (const int *)S.flag.p,
                     S.pos.p, S.next.p, stamp, S.ctl.p);
  if (!L.read_ctl(h)) return 0;
  if (hipGetLastError() != hipSuccess) { L.fail("walk launch"); return 0; }
  if (h[MI_BADREC]) { L.fail("a neighbour across a face of a point's ball does not hold the point"); return 0; }
  if (h[MI_OVF] != 0xffffffffu) {
    L.fail("the ball of point " + std::to_string(h[MI_OVF]) + " has more than " + std::to_string(MI_LMAX - 2) +
           " tets (MMG3D_LMAX); the state is the layer's start");
    if (stats) {
      T.overflow_ip = h[MI_OVF];
      *stats = T;
    }
    return 0;
  }
  T.front = h[MI_NFRONT];
  // 2. the tets' histories against the layer-start marks
  if (ne > 0)
    hipLaunchKernelGGL(k_mi_tets, dim3(nbt), dim3(256), 0, s, tets, ne, (const int *)S.mark.p, (const int *)S.tmp.p,
                       (const int *)S.pos.p, stamp, m, 0, S.mark2.p, S.D.p, S.key1.p, S.key2.p, S.ctl.p);
  std::vector<unsigned> D((size_t)nold);
  if (!L.read_words(D.data(), (const unsigned *)S.D.p, (size_t)nold, "losses")) return 0;
  if (hipGetLastError() != hipSuccess) { L.fail("tets launch"); return 0; }
  // 3. the sequential loop never blocked iff no group would pass below nemin
  bool clean = true;
  for (int g = 0; g < nold; g++) clean = clean && (int64_t)S.negrp[g] - (int64_t)D[g] >= S.nemin[g];
  if (clean) {
    // 4. the events, then the commit
    if (ne > 0)
      hipLaunchKernelGGL(k_mi_tets, dim3(nbt), dim3(256), 0, s, tets, ne, (const int *)S.mark.p, (const int *)S.tmp.p,
                         (const int *)S.pos.p, stamp, m, 1, S.mark2.p, S.D.p, S.key1.p, S.key2.p, S.ctl.p);
    hipLaunchKernelGGL(k_mi_points, dim3(nbp), dim3(256), 0, s, np, m, (const unsigned long long *)S.key1.p,
                       (const unsigned long long *)S.key2.p, S.tmp.p, S.s.p, S.flag.p);
    if (ne > 0) S.mark.swap(S.mark2);
    for (int g = 0; g < nold; g++) S.negrp[g] -= (int)D[g];
  } else {
    T.blocked = 1;
    std::vector<int> grp(S.negrp);
    grp.insert(grp.end(), S.nemin.begin(), S.nemin.end());
    // the parallel pass's counts do not hold for this path
    unsigned z[MI_NCTL] = {0};
    z[MI_OVF] = 0xffffffffu;
    PMX_CK(L, hipMemcpyAsync(S.grp.p, grp.data(), sizeof(int) * grp.size(), hipMemcpyHostToDevice, s));
    PMX_CK(L, hipMemcpyAsync(S.ctl.p, z, sizeof z, hipMemcpyHostToDevice, s));
    PMX_CK(L, hipStreamSynchronize(s));
    // the front of the layer's start, ascending: the lane never scans the points
    if (!L.grow(S.front, (size_t)std::max<int64_t>(np, 1)) ||
        !L.select_flagged(S.cub, hipcub::CountingInputIterator<int>(1), (const int *)S.flag.p + 1, S.front.p,
                          S.ctl.p + MI_NLIST, np, "front list"))
      return 0;
    for (;;) {
      hipLaunchKernelGGL(k_mi_seq, dim3(1), dim3(64), 0, s, tets, (const int *)S.front.p, S.mark.p, S.tmp.p, S.s.p,
                         S.flag.p, (const int *)S.next.p, m, S.grp.p, nold, steps, S.ctl.p);
      if (!L.read_ctl(h)) return 0;
      if (hipGetLastError() != hipSuccess) { L.fail("sequential launch"); return 0; }
      T.seq_launches++;
      if (h[MI_SEQ_IP] >= h[MI_NLIST]) break;
    }
    if (!L.read_words(S.negrp.data(), (const int *)S.grp.p, (size_t)nold, "negrp")) return 0;
  }
  // 5. / 6. the side fronts and the next front
  hipLaunchKernelGGL(k_mi_side, dim3(nbw), dim3(64), 0, s, np, (const int *)S.mark.p, m, (const int *)S.next.p,
                     S.tmp.p, S.s.p, S.flag.p, S.ctl.p);
  double ms = -1.0;
  if (!L.read_ctl(h) || !L.elapsed(ms)) return 0;
  ctx->moveifc_layer_ms = ms;
  T.touched = h[MI_TOUCHED];
  T.recolor = h[MI_NREC];
  T.next = h[MI_NEXT];
  T.blocks = h[MI_BLOCKS];
  T.maxball = h[MI_MAXBALL];
  if (stats) *stats = T;
  return 1;
}

int pmx_moveifc_marks(pmx_ctx *ctx, int32_t *mark) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_marks"};
  if (!L.live()) return 0;
  if (!mark) { L.fail("mark is NULL"); return 0; }
  const int64_t ne = L.st->ne;
  if (ne == 0) return 1;
  // through the pinned arena: the caller's array is written only after the copy succeeded
  const int32_t *h = (const int32_t *)pmx_hstage(ctx, sizeof(int32_t) * (size_t)ne);
  if (!h) return 0;
  if (!L.ok(hipMemcpyAsync((void *)h, L.st->mark.p + 1, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost, L.s),
            "marks download") ||
      !L.sync("marks download"))
    return 0;
  par_for(0, ne, [&](int64_t a, int64_t b) { std::copy(h + a, h + b, mark + a); });
  return 1;
}

int pmx_moveifc_points(pmx_ctx *ctx, int *tmp, int *s, int *front) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_points"};
  if (!L.live()) return 0;
  const pmx_moveifc_state &S = *L.st;
  const size_t n = (size_t)S.np;
  std::vector<int> a(tmp ? n : 0), b(s ? n : 0), c(front ? n : 0);
  if (!L.down(tmp ? a.data() : nullptr, (const int *)S.tmp.p + 1, S.np) ||
      !L.down(s ? b.data() : nullptr, (const int *)S.s.p + 1, S.np) ||
      !L.down(front ? c.data() : nullptr, (const int *)S.flag.p + 1, S.np) || !L.sync("points download"))
    return 0;
  if (tmp) std::copy(a.begin(), a.end(), tmp);
  if (s) std::copy(b.begin(), b.end(), s);
  if (front) std::copy(c.begin(), c.end(), front);
  return 1;
}

int pmx_moveifc_groups(pmx_ctx *ctx, int *negrp, int *nemin) {
  if (!ctx) return 0;
  MoveIfc L{ctx, "pmx_moveifc_groups"};
  if (!L.live()) return 0;
  if (negrp) std::copy(L.st->negrp.begin(), L.st->negrp.end(), negrp);
  if (nemin) std::copy(L.st->nemin.begin(), L.st->nemin.end(), nemin);
  return 1;
}

int pmx_moveifc_part(pmx_ctx *ctx, const int32_t *mark, int target, const int *ngrps_all, int32_t *part,
                     int32_t *ngrp) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  MoveIfc L{ctx, "pmx_moveifc_part"};
  if (!L.live()) return 0;
  const pmx_moveifc_state &S = *L.st;
  if (!part) { L.fail("part is NULL"); return 0; }
  if (target != PMX_GRPSPL_DISTR_TARGET && target != PMX_GRPSPL_MMG_TARGET) { L.fail("unknown target"); return 0; }
  const int64_t ne = S.ne;
  const int nprocs = S.nprocs;
  if (!mark) {
    // the device's marks: the partition's kernels into its scratch (the held
    // partition stays as it is), then one download through the pinned arena
    DevBuf<int> &d = ctx->partition.next;
    std::vector<int> group_mark;
    int n = 0;
    if (!pmx_part_of_marks(ctx, L.who, target, ngrps_all, d, &n, group_mark, nullptr)) return 0;
    if (ne > 0) {
      const int32_t *h = (const int32_t *)pmx_hstage(ctx, sizeof(int32_t) * (size_t)ne);
      if (!h) return 0;
      if (!L.down((int32_t *)h, (const int32_t *)d.p + 1, ne) || !L.sync("part download")) return 0;
      par_for(0, ne, [&](int64_t a, int64_t b) { std::copy(h + a, h + b, part + a); });
    }
    if (ngrp) *ngrp = n;
    return 1;
  }
  std::vector<int32_t> out((size_t)ne);
  if (target == PMX_GRPSPL_MMG_TARGET) {
    for (int64_t k = 0; k < ne; k++) {
      if (mark[k] < 0 || mark[k] % nprocs != S.myrank || mark[k] / nprocs >= S.nold) {
        L.fail("a mark of another rank's group (PMMG_GRPSPL_MMG_TARGET wants local marks)");
        return 0;
      }
      out[(size_t)k] = mark[k] / nprocs;
    }
    std::copy(out.begin(), out.end(), part);
    if (ngrp) *ngrp = S.nold;
    return 1;
  }
  // the compacted numbering: ranks visited from myrank round, the first used colour is group 0
  std::vector<int64_t> sum((size_t)nprocs + 1, 0);
  for (int r = 0; r < nprocs; r++) {
    const int n = ngrps_all ? ngrps_all[r] : S.displs[r + 1] - S.displs[r];
    if (n < 0) { L.fail("ngrps_all < 0"); return 0; }
    sum[r + 1] = sum[r] + n;
  }
  std::vector<int> used((size_t)sum[nprocs] + 1, 0);
  for (int64_t k = 0; k < ne; k++) {
    const int c = mark[k];
    if (c < 0 || c / nprocs >= sum[c % nprocs + 1] - sum[c % nprocs]) { L.fail("a mark of no group"); return 0; }
    out[(size_t)k] = (int32_t)(c / nprocs + sum[c % nprocs]);
    used[out[(size_t)k]] = 1;
  }
  int count = 0;
  for (int i = 0; i < nprocs; i++) {
    const int r = (i + S.myrank) % nprocs;
    for (int64_t c = sum[r]; c < sum[r + 1]; c++)
      if (used[c]) used[c] = count++;
  }
  for (int64_t k = 0; k < ne; k++) part[k] = used[out[(size_t)k]];
  if (ngrp) *ngrp = count;
  return 1;
}

int pmx_moveifc_release(pmx_ctx *ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  pmx_moveifc_free(ctx);
  return 1;
}

}  // extern "C"
