// pmx_kernels.h -- the argument blocks the kernels share and the launchers
// called across source files (host <-> device), by defining source.
#pragma once
#include "pmx_device.h"

struct GridDesc {
  int dim[3];
  double lo[3];
  double inv[3];
  int qf[3];        // fraction bits of the fixed-point grid coordinates:
                    // dim << qf fits 21 bits (qf = 21 - ceil(log2 dim))
};

// cell (x, y, z) of the volume hint grid, row-major.  (r03: 4x4x4 blocks of
// 64 cells, so that a wave of Morton-ordered points reads its hint cells from
// a few lines, left the walk within 0.5 % and made the surface path overlap it
// worse: C3 step 2.09 -> 2.19 ms, profiles/r03_c3_sweep_grid_priority.log.)
__host__ __device__ inline int64_t gcell(const GridDesc &g, int x, int y, int z) {
  return (int64_t)x + (int64_t)g.dim[0] * ((int64_t)y + (int64_t)g.dim[1] * z);
}

// counters of one step (d_counts, zeroed by the prologue):
//   [0] volume stuck, [1] surface stuck, [2] surface overflow, [3] volume ties,
//   [4] k_fallback grid-barrier arrivals, [7] device error flags (PMX_DERR_*)
#define PMX_CNT_ERR 7
#define PMX_DERR_BARRIER 1u         // a grid barrier gave up waiting (co-residency lost)

struct VolArgs {
  const double *xyz;            // old vertices, 24 B (x, y, z), 1-based
  const TetRec *tets;
  const WRec *wrec;             // the walk's compact copy of tets (null: walk on tets)
  const double *sol;
  SolDesc sd;
  const double *q;              // new points as uploaded, dense x y z (0-based)
  const int8_t *kind;
  int64_t nq, ne;
  const int *grid;              // hint grid, cell -> tet.  A PMX_RUN_POINTMAP step has none: it
                                // passes the start elements resolved by k_cls_write here,
                                // [0, nq) per volume list entry, [nq, 2 nq) per surface list
                                // entry, read by the PM instantiations of the walks (the
                                // argument block, and with it every default kernel, unchanged)
  GridDesc g;
  double *out;
  uint8_t *wmask;
  int *elem, *status, *steps, *start;
  int *stuck_list;
  unsigned *stuck_count;
  int2 *tie_list;               // (point, found tet) of points near a face
  unsigned *tie_count;
  int *found, *bestk;
  unsigned long long *best;
  const int *list;              // indices of the volume points (input order kept)
  int64_t nlist;                // upper bound (launch size); the step's count is *nlist_dev
  const int *nlist_dev;
  uint4 *wstats;                // per-wave {located, sum steps, max, min}
  int max_walk;
  unsigned const_bit;           // wmask bit of a constant-size metric (0 if none)
  int inline_ties;              // resolve face ties in place
  int ref_walk;                 // 1: k_walk (reference-order walk) instead of k_walks
  int rec_start;                // write the start tet of every point (diagnostics)
  int far;                      // the compact records have far neighbour fields (pmx_wrec.h)
  int exp;                      // run-flag experiment (pmx_internal.h): 0 production,
                                // 6 walk on the 32-B records,
                                // 17 a record with a far neighbour field read whole,
                                // 18 compact records whatever their far fields
};

// the surface kernels' arguments (pmx_bdy.hip; filled by bdy_args, pmx_internal.h)
struct BdyArgs {
  const double *xyz;        // old vertices, 24 B
  const TriRec *tris;
  const Pt4 *trn;
  const int2 *ntrange;      // fan [lo, hi) in ntlist of vertex l of tria k, at 3 k + l
  const int *ntlist;
  const double *sol;
  SolDesc sd;
  const double *q;          // new points, dense x y z (0-based)
  const int8_t *kind;
  int64_t nq, nt;
  double hausd;
  const int *grid;     // tria hint grid (shares GridDesc with the tet grid); a
                       // PMX_RUN_POINTMAP step: the start tria of every list entry
  GridDesc g;
  double *out;
  uint8_t *wmask;
  int *elem, *status, *steps, *start, *edge, *vertex;
  Pt4 *bphi;           // (non-null, nlist entries) per entry of `list`: the 3 barycentrics the point's fields were
                       // interpolated with, in the tria's vertex order (pmx_interp_more)
  int *stuck_list;     // bdy exhaustive list
  unsigned *stuck_count;
  int *ovf_list;       // private-list overflow
  unsigned *ovf_count;
  const int *list;       // indices of the boundary points
  int64_t nlist;         // upper bound (launch size); the step's count is *nlist_dev
  const int *nlist_dev;
  uint4 *wstats;         // per-wave walk statistics
  // PMX_RUN_SEQUENTIAL_SURFACE's speculative pass: per point its start tria
  // and mesh->base (null: the hint tria, ordinal + 1), and whether the walk
  // ran a shadow-wedge test (the only path to the point flags)
  const int *seq_start, *seq_base;
  uint8_t *seq_w;
};

struct ExhArgs {
  const double *xyz;
  const TetRec *tets;
  int64_t ne;
  const double *q;
  const int *list;
  const unsigned *count;
  int *found;
  unsigned long long *best;
  int *bestk;
  long spin_limit;              // grid-barrier poll budget (debug: 0 forces a timeout)
};

// ---- pmx_capi.hip ------------------------------------------------------------------

// constant-size metric (MMG3D_Set_constantSize restated): all valid points
void launch_const_metric(const int8_t *kind, int64_t nq, double *out, int S, int off, int size,
                         double hsiz, uint8_t *wmask, int imet, hipStream_t s);

// ---- pmx_background.hip ------------------------------------------------------------

// rows the step did not write: the caller's values, n entries (row, offset,
// size) + 6 doubles each, into the rows of S doubles at sol
void launch_patch_rows(const int4 *ent, const double *vals, int64_t n, int S, double *sol, hipStream_t s);

// ---- pmx_starts.hip ----------------------------------------------------------------

// per-background derived data: fixed-point grid coordinates of the vertices
// (hint centroids) and the unit normals of the boundary trias
// (PMMG_precompute_triaNormals, src/locate_pmmg.c:68-90), one launch
void launch_bg_derive(const double *xyz, int64_t np, GridDesc g, unsigned long long *xyzq,
                      const TriRec *tris, int64_t nt, Pt4 *trn, hipStream_t s);
// volume hint grid from every stride-th tet: `packed` = the host-packed
// connectivity of tets 1, 1+stride, ... (stride == PMX_HINT_STRIDE), else the
// tet records are read strided
void launch_hint_build(const int4 *packed, const int *kidx, const TetRec *tets, int64_t ne, int stride, int *grid,
                       GridDesc g, const unsigned long long *xyzq, hipStream_t s, int64_t nsamp = -1);
// the vertex-owner sample (k_vmin_owner): out[i] / kidx[i] the i-th vertex's
// owner tet in vertex order; owner np + 1 words, flag and pos np + 1 ints each,
// tmp owner_scan_temp_bytes(np) bytes; the sample count into *h_count (pinned)
size_t owner_scan_temp_bytes(int64_t np);
bool launch_owner_sample(const TetRec *tets, int64_t ne, int64_t np, unsigned *owner, int *flag, int *pos,
                         int4 *out, int *kidx, unsigned *d_count, unsigned *h_count, void *tmp, size_t tmp_bytes,
                         hipStream_t s);
// PMX_RUN_POINTMAP.  The first-incident-element maps of a background
// (PMMG_locate_setStart, src/locate_pmmg.c:931-986, whose loops keep the
// first index that reaches a vertex): map[p] = the smallest valid tet
// (v[0] > 0) holding vertex p, map[np + 1 + p] = the smallest tria, 0xffffffff
// when none; 2 (np + 1) words, filled here.  cnt[0..1]: atomics issued.
void launch_pmap_build(const TetRec *tets, int64_t ne, const TriRec *tris, int64_t nt, int64_t np,
                       unsigned *map, unsigned *cnt, hipStream_t s);

// ---- pmx_fallback.hip --------------------------------------------------------------

// the near-face ties (k_ties), then the exhaustive scan of the stuck points
// (k_fallback) on `blocks` co-resident workgroups
void launch_exhaustive(const ExhArgs &e, const VolArgs &v, int blocks, hipStream_t s);
// workgroups of k_fallback that can be co-resident with `share` other
// launches of it on this device (0 on error)
int fallback_coresident_blocks(int device, int share);

// ---- pmx_walk.hip ------------------------------------------------------------------

// the volume walk; pointmap: the PM instantiations (a.grid holds the start elements)
void launch_walk(const VolArgs &a, hipStream_t s, bool pointmap = false);
// PMX_RUN_SEQUENTIAL_VOLUME: the volume sequence (point
// indices in the reference's visit order, its length on the device), each
// point's speculative start and mesh->base, the speculation's "sure" flags,
// the replay's tet flags (ne + 1, base compare), its control words and
// one-point stuck list, the replay count
struct SeqVolArgs {
  const int *vseq;
  const int *nvseq;
  const int *sstart, *sbase;
  uint8_t *sure;
  int *tf;
  int *ctl;
  int *stk_list;
  unsigned *nreplay;
  const int *cand, *ncand;   // the positions whose speculative start may be wrong (sorted)
};
// the speculative pass and its overflow pass (workspace: seqv_ovf_ws_ints() ints)
size_t seqv_ovf_ws_ints();
void launch_seqv_spec(const VolArgs &a, const SeqVolArgs &s, int64_t nmax, int *ws, hipStream_t st);
void launch_seqv_resolve(const VolArgs &a, const SeqVolArgs &s, hipStream_t st);
// flags[j] (j < nmax) = position j of the volume sequence must be checked by
// the replay: not sure, or its start is not its predecessor's speculative tet
void launch_seqv_flags(const VolArgs &a, const SeqVolArgs &s, int64_t nmax, uint8_t *flags, hipStream_t st);

// ---- pmx_bdy.hip -------------------------------------------------------------------

// The surface walks: k_locate_bdy, its private-list overflow
// pass on ovf_threads threads -- linear lists in ows (OVF_THREADS threads'
// worth, the step's) or, hashed, tables of GHS_WS_INTS zeroed ints per thread
// (the sequential mode's speculative pass, whose walks from the predecessors'
// trias overflow by the thousand) -- and the exhaustive scan of the stuck list
#define OVF_THREADS (64 * 64)
#define GHS_SLOTS 4096               // per hash table and thread; at most half of them used
#define GHS_WS_INTS (GHS_SLOTS * 6)  // visited trias (int2) + point flags (int4)
void launch_bdy_walks(const BdyArgs &B, int *ows, hipStream_t s, int ovf_threads = OVF_THREADS, bool hashed = false,
                      bool pointmap = false);
// k_exh_bdy on `blocks` workgroups, one stuck point each at a time
void launch_exh_bdy(const BdyArgs &B, int blocks, hipStream_t s);
// PMX_RUN_SEQUENTIAL_SURFACE's replay (k_seq_resolve): the
// surface sequence and its length on the device, each point's speculative
// start, mesh->base and wedge flag, the reference's tria flags (nt + 1, base
// compare) and point flags (np + 1, PF_INIT: still the incident-tria count
// PMMG_precompute_nodeTrias left), the control words, the one-point stuck
// list of a replayed walk that ends stuck, the replay count, the candidates
#define PF_INIT ((int)0x80808080)
struct SeqBdyArgs {
  const int *seq, *nseq;
  const int *sstart, *sbase;
  const uint8_t *sw;
  int *tf, *pf;
  int *ctl;
  int *stk_list;
  unsigned *stk_count;
  unsigned *nreplay;
  const int *cand, *ncand;   // the positions the replay must look at (sorted)
};
void launch_seq_resolve(const BdyArgs &B, const SeqBdyArgs &q, hipStream_t s);

// ---- pmx_quality.hip, pmx_lengths.hip, pmx_graph.hip (stat_args) -------------------

struct StatArgs {
  // vertex v at xyz[xstride * (v - vbase)] (background: dense xyz, stride 3,
  // base 0; new mesh: the uploaded Pt4 points, stride 4, base = first index);
  // its metric at sol[S * (v - vbase) + moff], its tag at ptag[v - vbase]
  const double *xyz;
  int xstride, vbase;
  const TetRec *tets;           // records with neighbours (background only)
  const int4 *tetv;             // connectivity stream (v only)
  int64_t ne;
  const double *sol;
  int S, msize, moff;
  const uint16_t *ptag;         // point tags or null (no ridge points)
  // quality with metRidTyp = 1 and a tensor metric (MMG5_caltet_ani): the
  // mean metric leaves out the non-singular ridge points of these tags
  // (null: every vertex counts)
  const uint16_t *rtag;
  int ridmet;
  // edge lengths in a tensor metric along the curved surface (pmx_upload_surface;
  // null: no xTetra, zero normals): per tet the xTetra edge tags (bit 2 ia
  // MG_BDY, 2 ia + 1 MG_GEO), per point MMG5_Point.n and its xPoint index,
  // per xPoint n1 | n2 (6 doubles, entry 0 zero)
  const uint16_t *etag;
  const double *pn, *xpn;
  const int *pxp;
  // distributed prilen: sorted (min << 32 | max) keys of the parallel edges
  // the tet loop must skip, and a per-point prefilter
  const unsigned long long *par_key;
  int64_t npar;
  const uint8_t *par_pt;
};
