// pmx_internal.h -- the context object behind the C ABI (host only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>
#include "pmx_transfer.h"
#include "pmx_kernels.h"
#include "pmx_host.h"
#include "pmx_hostpool.h"

// hint grid from every 4th tet: 1/4 of the stores and of the tet bytes of a
// full build, at ~0.5 extra walk step (r01 measurements)
#define PMX_HINT_STRIDE 4
// pmx_run_opts.flags bits 16-23: the run-flag experiment (VolArgs.exp): 6, 17, 18
#define PMX_RUN_EXP_SHIFT 16
// the walk takes the 32-B tet records instead of the compact ones when more
// than 1/PMX_WREC_FAR_DIV of the tets have a far neighbour field (pmx_wrec.h)
#define PMX_WREC_FAR_DIV 16

// Slots of pmx_ctx::h_nbad (pinned words the device writes in stream order,
// valid on the host after a sync of that stream) and of pmx_ctx::d_wfar (their
// device counters).  "next" is the residency build's record set.
enum {
  PMX_H_NONMANIFOLD_NEXT = 0,   // non-manifold tet faces of the next record set's face matching
  PMX_H_NONMANIFOLD = 1,        // ... of the current one's (upload, adopt, promote, FRESH step)
  PMX_H_FAR = 2,                // tets of d_wrec with a far neighbour field (pmx_wrec.h)
  PMX_H_FAR_NEXT = 3,           // ... of d_wrec_next
  PMX_H_BAD_FANS = 4,           // check_fans: vertices whose fan the rotation cannot build
  PMX_H_NSAMP = 5,              // entries of the vertex-owner hint sample
  PMX_H_BAD_TRIAS = 6,          // device-built trias outside stage_trias' ranges (0 for the host's trias)
  PMX_H_WORDS = 8
};
enum {
  PMX_D_FAR = 0,                // far-field counter of d_wrec
  PMX_D_FAR_NEXT = 1,           // ... of d_wrec_next
  PMX_D_FANS_STEP = 2,          // bad fans of the step's rotation
  PMX_D_FANS_CHECK = 3,         // ... of the upload's check
  PMX_D_NSAMP = 4,              // owner-sample count
  PMX_D_BAD_TRIAS = 5,          // k_tri_records' range check
  PMX_D_WORDS = 8
};

// The device buffers of one boundary build (pmx_bdry_device, pmx_topo.hip):
// the trias (3 (nt + 1) ints, Mmg layout, row 0 zero) and their adjt
// (3 nt + 4 ints), then the scratch -- boundary faces per tet and their scan,
// edge buckets, edge records, the bucket of every record, one scan scratch
// per scan (no free while the first is queued)
struct BdryDev {
  DevBuf<int> tria, adjt, bof;
  DevBuf<unsigned> tcnt, tpos, cnt, off;
  DevBuf<int2> rec;
  DevBuf<char> tmp, tmp2;
};

// Where build_records puts a background's tet records: the buffers, the
// d_wfar slot of the compact records' far counter and the h_nbad slots of the
// non-manifold and far counts (pmx_ctx::records_current / records_next)
struct RecordSet {
  DevBuf<TetRec> *tets;
  DevBuf<WRec> *wrec;
  DevBuf<int4> *sample;
  int d_far, h_nonmanifold, h_far;
};

// The new mesh's tets on the device and the orphan reset that depends on
// them: one owner.  Other files read have / n / d_v and call the functions;
// only pmx_points.hip assigns a member.
//
//   the tets   none            !have
//              view kept       have, from_view, pending: `view` names the caller's rows, nothing is packed
//              DMA in flight   have, inflight: packed into h, the copies (and marks) issued on `up`, ev recorded
//              on the device   have, !pending, !inflight
//   the marks  valid or not    marks: d_mark[j] = 1 where a valid current tet holds point j
//   the rows   reset or not    rows_reset: the last step's rows of orphan points are "never visited" again
//   next       none, building  next_topo: the next background's records being built from the tets on `topo`
//
//   transition          called by                       the tets                marks      rows
//   points_begin        pmx_upload_points, first        none, drained; next dropped  not valid  reset
//   view_kept           pmx_upload_points, last         view kept (none without tets)
//   pack_new_tets       the end of the view's first     DMA in flight; next     valid      .
//                       step; ensure_tets before it     building with residency
//   replace             pmx_upload_new_tets             on the device; next     valid if   not reset if a
//                                                       dropped                 from_view  step has run
//   step_marks          a FRESH step with tets          DMA in flight           (being redone on `up`)
//   step_done(true)     ... its end                     .                       valid      reset: never located
//   step_done(false)    the end of any other step       .                       .          not reset
//   fix_orphans         every consumer of results       .                       .          reset
//   drain               points_begin, replace           in flight -> on the device
//   drop_next           points_begin, replace           .                       next: none
//   take_next           pmx_promote_background          .                       next: none (swapped in when wanted)
//   consumed            ... its end                     none
struct NewTets {
  pmx_ctx *const ctx;
  bool have = false;                    // there are new tets for the current points
  int64_t n = 0;                        // ne of them; records 1..n, vertex = points-view index - first + 1
  bool from_view = false;               // the points view carried them (orphans exist by definition)
  bool pending = false, inflight = false;
  bool marks = false, rows_reset = true;
  bool next_topo = false;
  pmx_points_view view{};
  DevBuf<int4> d_v;                     // the tets, 1-based, slot 0 unused
  DevBuf<uint8_t> d_mark;               // orphan marks, one byte per point
  PinBuf<char> h;                       // pinned copy of the tets (int4, 0 = deleted); not the shared arena:
                                        // it outlives the step (a strided quality output reads validity there)
  DevEvent ev, ev_topo;                 // the DMA and marks on `up`; the residency build on `topo`
  unsigned const_bit = 0;               // wmask bit of the last step's constant-size metric (kept by the reset)

  explicit NewTets(pmx_ctx *c) : ctx(c) {}
  bool points_begin();
  void view_kept(const pmx_points_view &pv, int64_t ntet);
  // the pending tets: validated, packed, sent on `up` in chunks, marked there;
  // with residency the next background's records follow on `topo`
  bool pack_new_tets();
  bool replace(const int *tetra_v, int64_t tetra_stride, int64_t ne);
  bool step_marks(hipStream_t st);      // the marks again on `up`, forked from st (which waits for ev later)
  void step_done(bool marks_in_step, unsigned step_const_bit);
  bool drain();                         // wait for ev on the host
  bool drop_next();                     // wait for `topo` on the host
  bool take_next(bool wanted);          // true: the prepared records are to be swapped in (after ev_topo)
  void consumed();                      // a promotion took them: none
  bool ensure_tets(hipStream_t s);      // d_v valid for work on stream s (packs a pending view)
  // the marks from d_v[1..ne] on stream s: d_mark[j] = 1 when a valid new tet
  // holds point j (the reference's vertex loop, src/interpmesh_pmmg.c:535-541)
  bool mark_new_tets(int64_t ne, hipStream_t s);
  // the last step located every live point; its rows of orphan points go back
  // to untouched on the context's stream, before any consumer reads them
  bool fix_orphans();
  int4 *grow_htets(int64_t ne);         // h for ne + 1 records (ev already waited for)
};

// The context's partition (pmx_part_*, pmx_part.hip): what the displacement's
// marks or the host's Metis array stand for, between the fix and the split.
// part: ne + 1 ints, tet k at k, as pmx_split_plan reads it; next: the one a
// call builds, swapped in when the call succeeded, so that a refusal leaves
// the held partition alone (and the scratch of pmx_moveifc_part(mark = NULL));
// tab: the colour table of the DISTR target -- sum (nprocs + 1), then the used
// flags that become the pack map; ctl: {bad marks, the smallest offending tet}.
// group_mark[g]: the mark of every tet of group g, empty after an upload.
struct pmx_partition {
  DevBuf<int> part, next, tab;
  DevBuf<unsigned> ctl;
  std::vector<int> group_mark;
  int ngrp = 0;
  bool valid = false;
  DevEvent ev[2];
  double ms = -1.0;                     // pmx_kernel_ms(ctx, 24)
};

struct pmx_ctx {
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  // the surface path runs on `side`, forked once the points are classified
  // and joined before the fallback: it overlaps the hint build and the volume walk
  hipStream_t side = nullptr;
  DevEvent ev_fork, ev_fork2, ev_join;
  DevEvent ev_dl[8];                    // chunked download: one per chunk
  std::string err;
  int fallback_blocks = 0;              // co-resident k_fallback workgroups
  int fallback_share = 0;               // live contexts on the device they were sized for
  // PMX_interpMetricsAndFields: a second context on the same device, groups
  // alternate between the two (created on first use, destroyed with this one)
  pmx_ctx *peer = nullptr;
  // pinned host staging arena (hipHostMalloc, grown on demand, reused across
  // steps): uploads and downloads go through it as async DMA
  PinBuf<char> h_stage;

  // background group (raw uploads)
  bool have_bg = false;
  int64_t np = 0, ne = 0, nt = 0;
  double hausd = 0.0;
  SolDesc sd{};
  GridDesc grid{};
  int64_t gcells = 0;
  double bblo[3]{}, bbhi[3]{};
  DevBuf<double> d_xyz;                 // old vertices, x y z (24 B), slot 0 unused
  DevBuf<TetRec> d_tets;
  DevBuf<WRec> d_wrec;                  // the walk's compact copy of d_tets (built with it)
  DevBuf<unsigned> d_wfar;              // device counters, PMX_D_WORDS of them: the PMX_D_* slots above
  DevBuf<double> d_sol;
  DevBuf<int4> d_tets_s;                // hint sample: every 4th tet (default, packed with the tets) or one owner tet per vertex (order_hint_samples)
  DevBuf<int> d_tets_sk;                // its tet indices (samples_sorted)
  bool samples_sorted = false;
  bool samples_owner = false;           // the vertex-owner sample: nsamp entries
  // decided at each background upload / promotion (environment, A/B):
  // compact_recs -- the walk's 24-B records d_wrec are built (PMX_WALK_RECORDS=compact;
  //   default: the walk reads the 32-B records, no per-background pass);
  // sample_mode -- PMX_HINT_SAMPLE_ORDER: 0 (default) every 4th tet, packed by the host
  //   with the tet records (or by k_build_tetrec), 2 one owner tet per vertex (device passes)
  bool compact_recs = false;
  int sample_mode = 0;
  // d_btv holds this background's raw connectivity and its adjacency was
  // built on the device (an upload without Mmg's adja)
  bool bg_btv = false;
  int64_t nsamp = 0;
  DevBuf<unsigned> d_skey;              // order_hint_samples scratch: keys / owners, indices / flags, records, temp
  DevBuf<int> d_sidx;
  DevBuf<int4> d_salt;
  DevBuf<char> d_stmp;
  DevBuf<TriRec> d_tris;
  // node -> trias fans (built on the device, in the step): ntlist = trias
  // sorted by (vertex, index), ntrange[3 k + l] = the run of vertex l of tria k
  DevBuf<int> d_ntlist, d_ntval;
  DevBuf<unsigned> d_ntkey;
  DevBuf<int2> d_ntrange;
  DevBuf<char> d_nttmp;
  bool have_csr = false;
  // derived from the raw uploads on the device (k_bg_derive), by the first
  // step after an upload or by every step with PMX_RUN_FRESH_BACKGROUND
  bool have_derived = false;
  DevBuf<unsigned long long> d_xyzq;    // fixed-point grid coordinates (hint centroids)
  DevBuf<Pt4> d_trn;                    // tria unit normals + areas
  DevBuf<int> d_grid;
  // PMX_RUN_POINTMAP: the first-incident-element maps (k_pmap_tets /
  // k_pmap_trias), np + 1 words each: [0, np] smallest valid tet holding the
  // vertex, [np + 1, 2 np + 1] smallest tria (0xffffffff: none).  Derived
  // background data, built by the first flagged step after an upload (or by
  // every flagged FRESH step), never by an unflagged one; d_pmcnt[0..1] the
  // atomics the two passes issued
  bool have_pmap = false;
  DevBuf<unsigned> d_pmap, d_pmcnt;
  // statistics only: 16-B connectivity stream, derived on first use
  bool have_tetv = false;
  DevBuf<int4> d_tetv;

  // new points and results
  bool have_pts = false, ran = false;
  int64_t nq = 0;
  // volume / surface point counts: upper bounds from the host's tag pass
  // (launch sizes); the exact counts are the step's classification (d_nsel)
  int64_t nq_vol_ub = 0, nq_bdy_ub = 0;
  int out_S = -1;                       // solution width the results were computed for
  int64_t out_n = -1;                   // point count the results were computed for
  // a step has run on the current points (each caller adds have_bg and
  // out_S == sd.S where it needs them)
  bool stepped() const { return ran && have_pts && out_n == nq; }
  DevBuf<int8_t> d_kind;
  DevBuf<uint8_t> d_wmask;
  DevBuf<double> d_out;
  DevBuf<int> d_elem, d_status, d_steps, d_start, d_edge, d_vertex;
  DevBuf<int> d_list, d_found, d_bestk;
  DevBuf<int2> d_ties;
  DevBuf<unsigned long long> d_best;
  DevBuf<unsigned> d_counts;            // step counters, see pmx_kernels.h
  DevBuf<int> d_vollist, d_bdylist;     // compacted point lists per path
  // per entry of d_bdylist (nq_bdy_ub of them): the barycentrics the located
  // surface point's fields were interpolated with
  DevBuf<Pt4> d_bphi;
  // pmx_interp_more (pmx_more.hip): the step located points (it had something
  // to interpolate), a batch's background rows, output rows and write masks
  // (reused across batches and calls), the batch kernels' events of the last call
  bool located = false;
  DevBuf<double> d_msol, d_mout;
  DevBuf<uint8_t> d_mwm;
  std::vector<DevEvent> more_ev;
  int more_ev_used = 0;
  DevBuf<double> d_qxyz;                // new points as uploaded (dense xyz)
  DevBuf<int> d_nsel;                   // compaction counts: volume, surface
  // the new points' source vertices (pmx_upload_point_sources; dense, entry
  // j = view index first + j) and, of a PMX_RUN_POINTMAP step, the resolved
  // start element per compacted point: [0, nq) volume list, [nq, 2 nq) surface
  bool have_src = false;
  DevBuf<int> d_qsrc, d_pstart;
  DevBuf<int2> d_ctile;                 // classification tile counts
  DevBuf<uint4> d_vstat, d_bstat;       // per-wave walk statistics
  DevBuf<int> d_blist, d_olist, d_ows;
  // PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME (pmx_seq.hip seq_replay): visit keys /
  // order, located / surface flags and their scan, bases | surface sequence |
  // volume sequence | speculative starts | control block, wedge / sure flags,
  // cub scratch, the replays' tria, point and tet flags, the volume
  // speculation's overflow workspace, the candidate flags and positions
  DevBuf<unsigned> d_sqkey;
  DevBuf<int> d_sqidx, d_sqint, d_sqtf, d_sqpf, d_sqtv, d_sqows;
  DevBuf<unsigned long long> d_sqval;
  DevBuf<uint8_t> d_sqw, d_sqflag;
  DevBuf<int> d_sqcand;                 // [0] count, then a replay's candidate positions
  DevBuf<char> d_sqtmp;
  unsigned seq_stats[4] = {0, 0, 0, 0};   // surface replays / sequence, volume replays / sequence
  int64_t seq_stats_n = -1;             // -1: the last step was not sequential
  DevBuf<int> d_tgrid;
  GridDesc tgd{};
  int64_t tcells = 0;
  // the last step built the volume / the tria hint grid (pmx_debug_grid): a
  // PMX_RUN_POINTMAP step builds neither, a step without surface points or
  // with nothing to locate no tria grid
  bool vgrid_built = false, tgrid_built = false;

  // group seams (pmx_groups.hip): constant-size metric of a step without a
  // background, and the frozen-point copy (buffers reused across calls)
  DevBuf<double> d_cmet;
  DevBuf<int> d_cperm, d_ccnt;         // pmx_copy_required

  // statistics
  DevBuf<double> d_qual;
  DevBuf<unsigned long long> d_red;
  bool have_qual = false;
  bool have_ptag = false;               // background point tags (pmx_upload_point_tags)
  DevBuf<uint16_t> d_ptag;
  // Mmg's surface data of the background (pmx_upload_surface): per tet the
  // xTetra edge tags packed 2 bits per edge (BDY, GEO); per point MMG5_Point.n
  // and its xPoint index; per xPoint n1, n2
  bool have_surf = false;
  DevBuf<uint16_t> d_etag;
  DevBuf<double> d_pn, d_xpn;
  DevBuf<int> d_pxp;
  DevBuf<uint16_t> d_pedge_tag;         // prilen: tags of the owned parallel edges
  // Metis element graph (pmx_metis_graph / pmx_face_weights): degrees (slot 0
  // = 0, so that their inclusive sum is xadj), xadj, adjncy, adjwgt, the
  // deleted-tet flag, cub scratch; the face list and its weights; the events
  // around the count, the scan and the fill of the last call (graph_ev_n of
  // them recorded: 0 none, 3 count + scan, 5 with a fill)
  DevBuf<int> d_gdeg, d_gxadj, d_gadj, d_gwgt, d_gface;
  DevBuf<unsigned> d_gflag;
  DevBuf<char> d_gtmp;
  DevBuf<double> d_gfw;
  DevEvent graph_ev[5];
  int graph_ev_n = 0;
  // Partition contiguity (pmx_contiguity / pmx_fix_contiguity, pmx_contig.hip),
  // ne + 1 words each: parents (labels once converged), marks, the replay's
  // visit stamps, its queues (the labelling's per-root sizes before that);
  // the component table, the replay records, the recolour list, the control
  // words {changed, bad record, deleted tet, roots, unfinished replays, replay
  // error}; the event pair and the summed times of the last call (-1: none)
  DevBuf<int> d_cpar, d_cmark, d_cstamp, d_cqueue;
  DevBuf<int4> d_ctab, d_crec;
  DevBuf<int2> d_crecol;
  DevBuf<unsigned> d_cctl;
  DevEvent contig_ev[2];
  double contig_label_ms = -1.0, contig_replay_ms = -1.0;
  // Group split (pmx_split_groups / pmx_split_fetch, pmx_split.hip): the plan
  // with its device buffers, valid until the next
  // background upload or promotion; device times of the last plan / fetch
  struct pmx_split_plan *split = nullptr;
  bool split_valid = false;
  double split_plan_ms = -1.0, split_fetch_ms = -1.0;
  // A device-resident group as this context's background (pmx_ctx_adopt_group;
  // pmx_split_adopt on the receiving context): the bounding-box reduction's
  // result and scratch, the boundary build's buffers, the event that orders
  // this stream behind the giving context's, the event pair and the device
  // time of the last pmx_split_adopt into this context
  DevBuf<double> d_bb;
  DevBuf<char> d_bbtmp;
  BdryDev bdry;
  DevEvent ev_give, adopt_ev[2];
  double split_adopt_ms = -1.0;
  // Group merge (pmx_merge_groups / _fetch / _maps / _adopt, pmx_merge.hip):
  // the plan with its device buffers, independent of the background (an
  // upload or a promotion leaves it alone); device times of the last plan /
  // fetch / adopt
  struct pmx_merge_plan *merge = nullptr;
  double merge_plan_ms = -1.0, merge_fetch_ms = -1.0, merge_adopt_ms = -1.0;
  // Interface displacement (pmx_moveifc_*, pmx_moveifc.hip): its state with
  // the device buffers, valid until the next background upload, promotion or
  // adoption; device times of the last begin / layer
  struct pmx_moveifc_state *moveifc = nullptr;
  bool moveifc_valid = false;
  double moveifc_begin_ms = -1.0, moveifc_layer_ms = -1.0;
  // Reachability (pmx_check_reachability / pmx_moveifc_fix / _reach,
  // pmx_reach.hip) works on d_cmark with the contiguity's parents, stamps,
  // queues, table, records and control words; its own: the tets' flags
  // (ne + 1), per root {seeded, size, start} (3 (ne + 1)), the sorted local
  // colours, the entries {face_index1 | colour received | gathered marks}, the
  // decisions {root, mark, flag} of a round.  moveifc_fixed: pmx_moveifc_fix
  // ran on the live displacement's marks and no layer or set_colors since;
  // moveifc_counter: its counter.  Device times of the last check / in-place fix
  DevBuf<int> d_rflag, d_raux, d_rcol, d_rface;
  DevBuf<int4> d_rdec;
  bool moveifc_fixed = false;
  int64_t moveifc_counter = 0;
  double reach_ms = -1.0, moveifc_fix_ms = -1.0;
  // The partition (pmx_part.hip), valid until the next background upload,
  // promotion or adoption (pmx_part_drop); pmx_moveifc_release leaves it
  pmx_partition partition;
  int64_t stat_np = -1;                // node count of pmx_count_nodes (-1: np)
  DevBuf<uint8_t> d_touch;
  DevBuf<int> d_cidx, d_intv;
  DevBuf<double> d_pub;                 // public partial records of the host wrappers
  DevBuf<unsigned long long> d_pkey;    // prilen: excluded parallel edges (sorted keys)
  DevBuf<uint8_t> d_ppt;
  DevBuf<int2> d_pedge;                 // prilen: owned parallel edges (step 1)
  double qlo[3]{}, qhi[3]{};            // bbox of the uploaded new points
  // device adjacency (pmx_topo.hip), reused buffers.  d_adja and the face
  // matching's scratch below are build_records' alone: one scratch shared by
  // the builds on the main and the topo stream, kept in order by ev_adja
  // (waited for before a build's first write, recorded after its last read;
  // created by the first build)
  DevBuf<int> d_adja;
  DevEvent ev_adja;
  DevBuf<int4> d_btv;                   // background connectivity when its adjacency is built here
  DevBuf<unsigned> d_tcnt, d_toff, d_tbad;
  DevBuf<int4> d_trec;
  DevBuf<char> d_ttmp;
  DevBuf<int4> d_pent;                  // promote: patched rows
  DevBuf<double> d_pval;
  // residency (pmx_set_residency): the next background's tet records, built
  // from the new tets on the `topo` stream while the current step runs
  bool residency = false;
  hipStream_t topo = nullptr;
  DevBuf<TetRec> d_tets_next;
  DevBuf<WRec> d_wrec_next;
  DevBuf<int4> d_tets_s_next;
  PinBuf<unsigned> h_nbad;              // pinned counts, PMX_H_WORDS of them: the PMX_H_* slots above
  DevBuf<double> d_nqual;
  bool have_qtag = false;               // raw tags of the new points
  DevBuf<uint16_t> d_qtag;
  int64_t pts_first = 0;                // points view's first index
  // the new tets' DMA and their orphan marks run on `up`, beside the step and
  // the results' download; the new tets themselves are `ntets`
  hipStream_t up = nullptr;
  NewTets ntets{this};
  // PMX_RUN_EAGER_DOWNLOAD: the last step's fields (n * S doubles) and write
  // masks (n bytes) copied into h_out as soon as the step ends, in eager_nch
  // chunks (ev_eg); 0 = no such copy, or the results changed since
  PinBuf<char> h_out;
  int eager_nch = 0;
  DevEvent ev_eg[4];
  DevBuf<double> d_gather;              // all-gathered partials

  // timing
  double topo_ms = 0.0;                 // device time of the last topology build
  std::vector<DevEvent> events;
  int ev_used = 0;

  ~pmx_ctx();                           // the split, merge and displacement plans (pmx_capi.hip); the members release themselves
  DevEvent *next_event_slot();          // nullptr + err on failure
  bool order_hint_samples(int64_t ne, int64_t nverts, hipStream_t s);
  // the background's record set, and the one the residency build prepares
  RecordSet records_current() { return {&d_tets, &d_wrec, &d_tets_s, PMX_D_FAR, PMX_H_NONMANIFOLD, PMX_H_FAR}; }
  RecordSet records_next() {
    return {&d_tets_next, &d_wrec_next, &d_tets_s_next, PMX_D_FAR_NEXT, PMX_H_NONMANIFOLD_NEXT, PMX_H_FAR_NEXT};
  }
  // Connectivity -> tet records on stream s (pmx_background.hip), the only
  // code that touches d_adja: the face matching of tv (1-based int4 on the
  // device, slot 0 unused) -- or, when the caller has Mmg's adjacency
  // (host_adja, 4 ne + 5 ints), its copy to the device --, then the 32-B
  // records with the every-4th-tet sample and, with compact_recs, the walk's
  // records; tv == nullptr: the 32-B records are in place, only the walk's
  // are built.  The destination buffers are grown; the counts land in dst's
  // h_nbad slots when s gets there.
  bool build_records(const int4 *tv, const int *host_adja, int64_t ne, int64_t np, const RecordSet &dst,
                     hipStream_t s);
  // PMX_RUN_FRESH_BACKGROUND: the per-background device passes of an upload
  // (face matching + records when the device built the adjacency, compact
  // records, owner sample), again on stream s (pmx_background.hip)
  bool rederive(hipStream_t s);
  // the node -> trias fans (pmx_fans.hip): by rotation (closed manifold
  // surface, checked at the upload: fan_rot) or by a sort
  bool fan_rot = false;
  bool fan_rotation(hipStream_t s, unsigned *d_bad, bool check = false);
  bool check_fans(hipStream_t s);
  // from d_tris, np, nt; check: the rotation also finds the vertices with
  // more than one fan, the upload's fan check (a FRESH step redoes it)
  bool build_node_trias(hipStream_t s, bool check = false);
  // the new points: kinds, lists (pmx_points.hip); marks: the orphan marks
  // (ntets.d_mark) classify points in no valid new tet as KIND_ORPH
  // pointmap: also the start element of every compacted point from its
  // source vertex (d_qsrc through d_pmap into d_pstart)
  bool classify(hipStream_t s, bool marks = false, bool pointmap = false);
  // the step's surface locate (pmx_bdy.hip); pointmap: a.grid holds the start
  // elements (no tria hint grid is built)
  bool launch_bdy(const VolArgs &a, hipStream_t s, bool pointmap = false);
  bool size_tria_grid();                  // tgd, tcells, d_tgrid from the background's bbox and nt (pmx_bdy.hip)
  // PMX_RUN_SEQUENTIAL_SURFACE / _VOLUME after the step's passes, on stream s
  // (synchronises the host: a replayed query that ends stuck is rescued by a
  // launch of its own; pmx_seq.hip)
  bool seq_replay(const VolArgs &a, hipStream_t s, bool surf, bool vol);
  bool eager_download();                  // issue the eager copies of the step just enqueued
  // device error word of the last step (after a stream sync): 0 = none
  bool check_device_errors();
};

inline void pmx_set_error(pmx_ctx *ctx, std::string msg) { ctx->err = std::move(msg); }
// the surface kernels' arguments for the step's points; pointmap: the start
// trias of a.grid instead of the tria hint grid (pmx_bdy.hip)
BdyArgs bdy_args(pmx_ctx *ctx, const VolArgs &a, bool pointmap = false);
// the context's pinned staging arena, at least `bytes`, once the context's
// stream has drained (pmx_capi.hip)
char *pmx_hstage(pmx_ctx *ctx, size_t bytes);
// qualities dev[0..ne] (stream order) into the caller's array: stride 8
// (dense) writes qual[0..ne] with qual[0] = 0; any other stride (bytes, an
// AoS field such as &MMG5_Tetra[0].qual) writes only the tets that are valid
// in ntets.h (deleted tets keep their value, as MMG3D_tetraQual skips
// !MG_EOK).  Chunked through the pinned arena, each chunk's host scatter
// overlapping the next one's DMA (pmx_results.hip).
bool pmx_download_qual(pmx_ctx *ctx, const double *dev, int64_t ne, double *qual, int64_t stride);
// streaming (non-temporal) 16-B stores into the pinned staging: the host
// never reads those lines again, and a plain store first reads each line for
// ownership (a third of the packing traffic).  A pass ends with a full fence
// before its DMA is issued.
typedef int pmx_v4i __attribute__((ext_vector_type(4)));
static inline void st4(int4 *p, int a, int b, int c, int d) {
  const pmx_v4i v = {a, b, c, d};
  __builtin_nontemporal_store(v, (pmx_v4i *)p);
}
// PMX_TRACE=1: host phase timings of the staging calls on stderr
struct Trace {
  const char *who;
  bool on;
  std::chrono::steady_clock::time_point t0, last;
  explicit Trace(const char *w) : who(w), on(getenv("PMX_TRACE") != nullptr) {
    if (on) t0 = last = std::chrono::steady_clock::now();
  }
  void mark(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[pmx] %s %-22s %8.3f ms\n", who, what,
            std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

// face adjacency of device connectivity (1-based int4, slot 0 unused) into
// dadja (Mmg layout, 4 ne + 5 ints), context-owned scratch; false on a
// non-manifold face or a failure (ctx->err).  Called by build_records only.
// h_nbad != NULL: asynchronous on stream s, the non-manifold count lands in
// *h_nbad (pinned) when the stream gets there; NULL: checked before returning
bool pmx_ctx_build_adja_device(pmx_ctx *ctx, const int4 *tv, int64_t ne, int64_t np, int *dadja,
                               hipStream_t s, unsigned *h_nbad);
extern "C" int pmx_timing_reset(pmx_ctx *ctx);
// pmx_kernel_ms(ctx, 7): the batch kernels of the last pmx_interp_more (pmx_more.hip)
double pmx_more_kernel_ms(pmx_ctx *ctx);
// pmx_kernel_ms(ctx, 8..11): the last pmx_metis_graph -- its kernels summed,
// the count, the scan, the fill (pmx_graph.hip)
double pmx_graph_kernel_ms(pmx_ctx *ctx, int which);
// Partial records per statistics pass, a function of ne only, and the width of
// the fixed-order final reduction's first level (pmx_quality.hip)
#define FINAL_GRID 64
int stat_blocks(int64_t ne);
// d_tetv, the quality pass's 16-B connectivity stream, derived from the tet
// records on first use after an upload (pmx_quality.hip)
bool ensure_tetv(pmx_ctx *ctx);
// the statistics' view of the uploaded group; tetv false: without d_tetv
// (pmx_quality.hip)
bool stat_args(const pmx_call &C, StatArgs &A, bool tetv = true);
// d_red, the passes' partial records, at least `bytes` (pmx_quality.hip)
bool ensure_red(pmx_ctx *ctx, size_t bytes);
// metRidTyp is 0 or 1 (pmx_quality.hip)
bool check_met_rid_typ(const pmx_call &C, int metRidTyp);
// The lengths' view of the group on A, after stat_args: ridge storage from
// metRidTyp and the metric size -- refused without the point tags --, the
// surface arrays when they are uploaded (pmx_lengths.hip)
bool length_view(const pmx_call &C, int metRidTyp, StatArgs &A);
// a public partial record as the statistics the host wrappers return (pmx_reduce.hip)
void qual_to_stats(const pmx_qual_part &r, pmx_qual_stats *st);
void len_to_stats(const pmx_len_part &r, pmx_len_stats *st);
// the public record (pmx_qual_part / pmx_len_part) that a host wrapper's
// device call left in d_pub, on the host
template <class R> inline bool read_pub(const pmx_call &C, R &r) {
  return C.read_words(&r, (const R *)C.ctx->d_pub.p, 1, "download");
}
// pmx_kernel_ms(ctx, 12 / 13): the labelling / the replay and recolour kernels
// of the last pmx_contiguity or pmx_fix_contiguity, summed (pmx_contig.hip)
double pmx_contig_kernel_ms(pmx_ctx *ctx, int which);
// pmx_fix_contiguity's loop on a device mark array (ne + 1 ints, slot 0
// unused): staged through d_cmark, written back when the fix succeeded; the
// dequeues per replay launch that replay_steps = 0 stands for (pmx_contig.hip)
bool pmx_contig_fix_device(pmx_ctx *ctx, const char *who, int *d_mark, int32_t ncolors, const int32_t *colors,
                           int64_t replay_steps, pmx_contig_stats *st);
int pmx_contig_default_replay_steps();
// pmx_kernel_ms(ctx, 22 / 23): the last reachability check / in-place fix (pmx_reach.hip)
double pmx_reach_kernel_ms(pmx_ctx *ctx, int which);
// pmx_kernel_ms(ctx, 14 / 15 / 21): the last split plan / the last fetch / the
// last pmx_split_adopt into ctx; the plan and its buffers freed (pmx_split.hip)
double pmx_split_kernel_ms(pmx_ctx *ctx, int which);
void pmx_split_free(pmx_ctx *ctx);
// pmx_kernel_ms(ctx, 16 / 17 / 18): the last merge plan / fetch / adopt; the
// plan and its buffers freed (pmx_merge.hip)
double pmx_merge_kernel_ms(pmx_ctx *ctx, int which);
void pmx_merge_free(pmx_ctx *ctx);
// the live merge plan's tet_group on the device (ne ints, tet k at k - 1) and
// its tet count; false: no plan (pmx_merge.hip)
bool pmx_merge_tet_group(pmx_ctx *ctx, const int **tgrp, int64_t *ne);
// pmx_kernel_ms(ctx, 19 / 20): the last displacement begin / layer; the state
// and its buffers freed (pmx_moveifc.hip)
double pmx_moveifc_kernel_ms(pmx_ctx *ctx, int which);
void pmx_moveifc_free(pmx_ctx *ctx);
// the live displacement's marks on the device (ne + 1 ints, slot 0 unused)
// with its sizes; false: no live displacement (pmx_moveifc.hip)
struct MoveIfcMarks {
  int *mark;
  int64_t ne;
  int nprocs, myrank, nold;
  const int *displs;         // the map's displsgrp (host, nprocs + 1 ints)
};
bool pmx_moveifc_live_marks(pmx_ctx *ctx, MoveIfcMarks *m);
// pmx_kernel_ms(ctx, 24): the last pmx_part_from_marks (pmx_part.hip)
double pmx_part_kernel_ms(pmx_ctx *ctx);
// the held partition is no more: called by begin_background, that is by every
// install that drops the split plan and the displacement, and by the
// context's destructor (pmx_part.hip)
void pmx_part_drop(pmx_ctx *ctx);
// PMMG_part_getInterfaces on the live displacement's marks into dst (grown to
// ne + 1 ints, tet k at k) on the context's stream, which is synchronised.
// The held partition is not read or written: pmx_part_from_marks swaps dst in,
// pmx_moveifc_part(mark = NULL) downloads it.  group_mark: resized to *ngrp;
// ms (may be null): first to last device operation.  false + ctx->err, and
// dst's contents are undefined (pmx_part.hip)
bool pmx_part_of_marks(pmx_ctx *ctx, const char *who, int target, const int *ngrps_all, DevBuf<int> &dst,
                       int *ngrp, std::vector<int> &group_mark, double *ms);
// the held partition on the device (ne + 1 ints, tet k at k) and its group
// count; false: none (pmx_part.hip)
bool pmx_part_held(pmx_ctx *ctx, const int **part, int *ngrp);
// Boundary trias and their edge adjacency of device connectivity tv (1-based
// int4, slot 0 unused) into B, on C's stream (pmx_topo.hip): a face of a valid
// tet is a tria when its adjacency entry adj[adj_stride * k + adj_off + f] is 0
// (Mmg's adja: stride 4, off -3; the tet records' neighbour fields: 8, 4), in
// (tet, face) order, vertices in MMG5_idir order; with want_adjt an edge has a
// neighbour when exactly two trias share it.  *nt: their number (the stream
// is synchronised once to read it; more than maxnt fails before anything
// tria-sized is allocated).  e0 / e1 (may be null): recorded before the first
// and after the last kernel.
bool pmx_bdry_device(const pmx_call &C, const int4 *tv, const int *adj, int adj_stride, int adj_off, int64_t ne,
                     int64_t np, bool want_adjt, int64_t maxnt, BdryDev &B, int64_t *nt, hipEvent_t e0,
                     hipEvent_t e1);
// the bounding box of the rows 1..np of xyz (device, 24-B rows) on C's stream,
// which is synchronised; bb: 6 doubles, tmp: hipcub's scratch (pmx_background.hip)
bool pmx_bbox_device(const pmx_call &C, const double *xyz, int64_t np, DevBuf<double> &bb, DevBuf<char> &tmp,
                     double lo[3], double hi[3]);
// A group that is already on the device becomes the uploaded group, as
// pmx_upload_background with adja = NULL leaves it; the copies are device to
// device on the context stream (pmx_background.hip).  false + ctx->err, no
// background kept.
struct AdoptSrc {
  const int4 *tv;            // the tets 1..ne (tv[0] is tet 1)
  const double *xyz, *sol;   // source rows: row r at xyz + 3 r and sol + S r (interleaved solutions)
  const int *idx;            // nullptr: the group's row i is source row i, row 0 included;
                             // else its row i is source row idx[i - 1] (np entries) and row 0 is zeroed
  bool surface;              // false: nt = 0; true: the boundary trias and their adjacency are built
  double hausd;              // ... and this is the background's hausd
};
bool pmx_ctx_adopt_group(pmx_ctx *ctx, const char *who, const AdoptSrc &src, const SolDesc &sd, int64_t np,
                         int64_t ne);
// error of a call made without a context (pmx_last_error(NULL), per thread)
void pmx_set_noctx_error(const char *msg);
