// pmx_contig_dev.h -- the device helpers the labellings of pmx_contig.hip and
// pmx_reach.hip share: the control words, the parent trees' find and link, the
// kernels that start and flatten the trees.  Included inside each file's
// anonymous namespace.
#pragma once

// control words (d_cctl)
enum { CC_CHANGED = 0, CC_BADREC = 1, CC_DELETED = 2, CC_ROOTS = 3, CC_PENDING = 4, CC_RERR = 5, CC_NCTL = 8 };
#define CC_OPEN_BIT 0x80000000u
#define CC_DEFAULT_REPLAY_STEPS 1024

// parents to self, sizes to 0; a deleted tet raises ctl[CC_DELETED], a
// neighbour outside 0..ne ctl[CC_BADREC]
__global__ __launch_bounds__(256) void k_cc_init(const TetRec *__restrict__ tets, int64_t ne, int *__restrict__ par,
                                                 unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > ne) return;
  par[k] = (int)k;
  if (k == 0) return;
  const int4 *recs = reinterpret_cast<const int4 *>(tets);
  const int4 v = recs[2 * k], nb = recs[2 * k + 1];
  if (v.x <= 0) ctl[CC_DELETED] = 1u;
  const int n = (int)ne;
  if (nb.x < 0 || nb.x > n || nb.y < 0 || nb.y > n || nb.z < 0 || nb.z > n || nb.w < 0 || nb.w > n)
    ctl[CC_BADREC] = 1u;
}

// an ancestor of a that was its own parent when read
__device__ __forceinline__ int cc_find(const int *par, int a) {
  int p;
  while ((p = par[a]) != a) a = p;
  return a;
}

// link the trees of a and b: the larger node's parent goes down to the smaller
// node; when the atomic displaces another parent (or finds a smaller one), the
// pair (that parent, the smaller node) still has to be linked.  The larger
// node of the pair strictly decreases, so the loop ends.
__device__ __forceinline__ void cc_link(int *par, int a, int b) {
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(&par[hi], lo);
    if (old == hi || old == lo) break;
    a = old;
    b = lo;
  }
}

// no hooking runs beside it, so roots are stable and every tet ends on its
// root; nothing to do after a hooking launch that changed nothing
__global__ __launch_bounds__(256) void k_cc_jump(int64_t ne, int *par, const unsigned *__restrict__ ctl) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  if (k > ne || !ctl[CC_CHANGED]) return;
  const int r = cc_find(par, (int)k);
  if (par[k] != r) par[k] = r;
}
