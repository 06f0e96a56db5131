/*
 * pmx_transfer.h -- C ABI of the MI355X-native ParMmg transfer path.
 *
 * Replaces, behind ParMmg's own seams, the reference interface:
 *   PMMG_interpMetricsAndFields(PMMG_pParMesh, int *permNodGlob)
 *       reference src/parmmg.h:472, def src/interpmesh_pmmg.c:663-741,
 *       sole caller src/libparmmg1.c:829  -> PMX_interpMetricsAndFields
 *   PMMG_copyMetricsAndFields_point(...)
 *       reference src/parmmg.h:473, def src/interpmesh_pmmg.c:432-446,
 *       caller src/libparmmg1.c:792       -> PMX_copyMetricsAndFields_point
 *   PMMG_locatePointVol / PMMG_locatePointBdy (src/locate_pmmg.h:63-68) and
 *   PMMG_interp{4,3,2}bar_{iso,ani} selected by PMMG_setfunc
 *       (src/parmmgexterns.c:4-6, src/libparmmg_tools.c:595-612)
 *                                          -> pmx_run (batched, on device)
 *   PMMG_tetraQual / PMMG_qualhisto / PMMG_prilen (src/parmmg.h:564-566,
 *       def src/quality_pmmg.c:156-346,591-733)
 *                                          -> pmx_tetra_qual / pmx_qualhisto /
 *                                             pmx_prilen
 *   PMMG_graph_meshElts2metis / PMMG_computeWgt (src/metis_pmmg.c:746-823,
 *       280-301)                           -> pmx_metis_graph / pmx_face_weights
 *   PMMG_check_grps_contiguity / PMMG_check_part_contiguity
 *       (src/metis_pmmg.c:446-529, 312-392) -> pmx_contiguity
 *   PMMG_fix_contiguity_split / _centralized / PMMG_fix_contiguity
 *       (src/moveinterfaces_pmmg.c:377-611) -> pmx_fix_contiguity
 *   PMMG_split_eachGrp (src/grpsplit_pmmg.c:1267-1445)
 *                                          -> pmx_split_groups / pmx_split_fetch
 *   PMMG_update_oldGrps (src/libparmmg1.c:653) of a split's new group, with
 *   MMG5_chkBdryTria + MMG3D_hashTria (src/grpsplit_pmmg.c:400-414)
 *                                          -> pmx_split_adopt
 *   PMMG_merge_grps (src/mergemesh_pmmg.c:967-1073)
 *                                          -> pmx_merge_groups / pmx_merge_fetch /
 *                                             pmx_merge_adopt
 *   PMMG_set_color_tetra / PMMG_mark_interfacePoints /
 *   PMMG_part_moveInterfaces / PMMG_part_getInterfaces
 *       (src/moveinterfaces_pmmg.c:119-134, 1052-1090, 1306-1440, 1150-1212)
 *                                          -> pmx_moveifc_begin / _get_colors /
 *                                             _set_colors / _layer / _marks /
 *                                             _part
 *   PMMG_check_reachability (src/moveinterfaces_pmmg.c:627-811) -> pmx_reach_face_marks /
 *                                             pmx_check_reachability; with
 *   PMMG_fix_contiguity on the displacement's own marks (:1446-1452)
 *                                          -> pmx_moveifc_fix / pmx_moveifc_reach
 *   PMMG_part_getInterfaces (src/moveinterfaces_pmmg.c:1150-1212) or Metis's
 *   part[] after PMMG_fix_contiguity_split (:377-523), handed straight to
 *   PMMG_split_grps (src/grpsplit_pmmg.c:1680-1711), and the mark
 *   PMMG_part_getProcs (src/moveinterfaces_pmmg.c:1102-1118) reads off each
 *   new group                              -> pmx_part_from_marks / _upload /
 *                                             _download / _fix / _release,
 *                                             pmx_split_groups_part
 *
 * Rules (ParMmg conventions): plain C, pointers + sizes, no torch types.
 * Host memory is caller owned; device buffers are owned by the context.
 * Functions return 1 on success and 0 on failure (pmx_last_error() says why).
 * One host thread per context, one context per GPU (rank -> device by
 * rank % ndev).  Mesh arrays are 1-based exactly as in Mmg: slot 0 unused,
 * adja[4*(k-1)+1+f] = 4*k'+f', adjt[3*(k-1)+1+e] = 3*k'+e'.
 */
#ifndef PMX_TRANSFER_H
#define PMX_TRANSFER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_TAG_REQ   4        /* MG_REQ */
#define PMX_TAG_BDY   16       /* MG_BDY */
#define PMX_TAG_NUL   16384    /* MG_NUL */
#define PMX_MAX_SOLS  8        /* solutions of one fused step (and of a Medit
                                  file); further ones: pmx_interp_more */

typedef struct pmx_ctx pmx_ctx;

/* Strided view of an Mmg-style AoS mesh.  Pass e.g.
 *   point_c = &mesh->point[0].c[0], point_stride = sizeof(MMG5_Point),
 *   tetra_v = &mesh->tetra[0].v[0], tetra_stride = sizeof(MMG5_Tetra).
 * Strides are in BYTES.  Entries 1..n are read. */
typedef struct {
  int64_t       np, ne, nt;
  const double *point_c;  int64_t point_stride;
  const int    *tetra_v;  int64_t tetra_stride;
  const int    *adja;                       /* 4*ne+5 ints, may be NULL */
  const int    *tria_v;   int64_t tria_stride;
  const int    *adjt;                       /* 3*nt+4 ints, may be NULL  */
  double        hausd;                      /* mesh->info.hausd          */
} pmx_mesh_view;

/* A solution on the mesh vertices: m[size*ip + j], ip = 1..np (Mmg layout). */
typedef struct {
  int           size;     /* 1 scalar/iso metric, 3 vector, 6 tensor/ani metric */
  double       *m;
} pmx_sol_view;

/* New points to transfer onto: c[ip] at (const char*)c + ip*stride, ip=first..last;
 * tag as uint16_t at (const char*)tag + ip*tag_stride (MMG5_Point.tag).
 * Optional new tets (tetra_v != NULL, entries 1..ne, stride in bytes, vertex
 * indices in the same numbering as ip): only the points of valid tets
 * (v[0] > 0) are located, as in the reference's vertex loop over the new tets
 * (src/interpmesh_pmmg.c:535-541); the others are left untouched (a constant
 * size metric is still written on every valid point).  NULL: every point.
 * The tets also stay on the device (pmx_new_mesh_qual, pmx_promote_background).
 * They are read, validated and sent by the first pmx_run on these points,
 * once its step is enqueued (their DMA overlaps the step and the download; a
 * vertex outside [first, last] fails that pmx_run): the array must stay
 * valid until then. */
typedef struct {
  int64_t         first, last;
  const double   *c;    int64_t stride;
  const uint16_t *tag;  int64_t tag_stride;
  const int      *tetra_v;  int64_t tetra_stride;  int64_t ne;
} pmx_points_view;

/* Localisation statistics (reference PMMG_locateStats, src/locate_pmmg.h:45-50) */
typedef struct {
  int64_t nvol, nbdy;        /* located points by path            */
  int64_t nexhaust;          /* exhaustive searches               */
  int64_t nclosest;          /* not found -> closest element      */
  int64_t stepmin, stepmax;  /* |steps| over every located point, */
  double  stepav;            /* exhaustive ones included, as
                                PMMG_locate_postprocessing (src/locate_pmmg.c:
                                995-1028); an exhaustive point counts its walk
                                steps + 1 (the reference adds every tet it
                                scanned); no point: stepmin = the background's
                                ne, stepav 0                          */
} pmx_locate_stats;

/* ---- context ---------------------------------------------------------- */
/* A context owns one stream's device buffers and a pinned host staging arena
 * (hipHostMalloc, grown on demand, kept until pmx_destroy): about 36 B per
 * background tet + (24 + 8*S) B per background vertex, or 65 B per new vertex,
 * whichever upload is larger.  Host gathers/scatters of 2^18 elements or more
 * use PMX_HOST_THREADS threads (default min(8, hardware threads));
 * PMX_HOST_THREADS_MIN overrides that threshold. */
pmx_ctx    *pmx_create(int device);
void        pmx_destroy(pmx_ctx *ctx);
/* ctx == NULL: the last error of a call made without a context (this thread) */
const char *pmx_last_error(pmx_ctx *ctx);
/* Run on an external HIP stream (hipStream_t passed as void*); NULL = own. */
int         pmx_set_stream(pmx_ctx *ctx, void *hip_stream);
int         pmx_synchronize(pmx_ctx *ctx);
/* Device and build identification. */
int         pmx_device_info(pmx_ctx *ctx, char *buf, int buflen);

/* ---- background (old) group -------------------------------------------- */
/* AoS -> SoA conversion on the host, then upload.  imet = index of the
 * metric in sols[] (or -1).  If adja is NULL it is rebuilt from tetra_v by
 * device face matching (overlapped with the solutions' upload; half the tet
 * bytes over PCIe -- the faster choice for a valid conforming mesh, whose
 * face adjacency is unique; non-manifold faces fail the upload).
 * Every argument is checked before the context changes; on failure the
 * context holds no background (pmx_run refuses until a good upload). */
int pmx_upload_background(pmx_ctx *ctx, const pmx_mesh_view *old_mesh,
                          int nsol, const pmx_sol_view *old_sols, int imet);

/* ---- new points -------------------------------------------------------- */
int pmx_upload_points(pmx_ctx *ctx, const pmx_points_view *pts);

/* Source vertices of the new points (ParMmg's USE_POINTMAP build: Mmg gives
 * every new point the index of the background vertex it descends from,
 * MMG5_Point.src, seeded src = k before the remesh, src/libparmmg1.c:667-670).
 * Entry ip at (const char*)src + ip*stride, ip = first..last of the last
 * points view; pass &mesh->point[0].src, sizeof(MMG5_Point).  After
 * pmx_upload_points, kept until the next pmx_upload_points; src == NULL
 * forgets them.  Returns 0 when no points are uploaded.  Read by a pmx_run
 * with PMX_RUN_POINTMAP. */
int pmx_upload_point_sources(pmx_ctx *ctx, const int *src, int64_t stride);

/* ---- the hot path (device resident) ------------------------------------ */
typedef struct {
  int    hint_stride;              /* hint grid built from every k-th tet,
                                      0 -> default                           */
  int    max_walk;                 /* walk step cap before exhaustive, 0=auto */
  double hsiz;                     /* >0: constant-size metric shortcut
                                      (src/interpmesh_pmmg.c:497-512)        */
  int    timing;                   /* record per-kernel HIP events           */
  int    flags;                    /* PMX_RUN_* (0 = production defaults)    */
} pmx_run_opts;

/* pmx_run_opts.flags */
#define PMX_RUN_REFERENCE_WALK   0x1  /* volume walk in the reference's order
                                         (k_walk) instead of the slot walk    */
#define PMX_RUN_NO_INLINE_TIES   0x2  /* every near-face point to the tie BFS */
#define PMX_RUN_RECORD_STARTS    0x4  /* keep each volume walk's start tet    */
#define PMX_RUN_SERIAL_SURFACE   0x8  /* surface path on the main stream      */
#define PMX_RUN_FRESH_BACKGROUND 0x10 /* redo every device pass the uploads
                                         ran on the raw arrays (derived data,
                                         fan check, device-built layouts, the
                                         orphan marks of the new tets): one
                                         ParMmg iteration per step            */
#define PMX_RUN_SEQUENTIAL_SURFACE 0x40 /* the reference's SEQUENTIAL surface
                                         semantics (src/interpmesh_pmmg.c:
                                         528-599, src/locate_pmmg.c:209-334):
                                         the boundary points in the vertex
                                         loop's first-visit order through the
                                         new tets, each query starting from the
                                         previous one's tria, the point flags
                                         of the shadow cone / wedge tests and
                                         mesh->base carried over.  Needs the new
                                         tets (points view or
                                         pmx_upload_new_tets).  Default: every
                                         query fresh from its hint tria        */
#define PMX_RUN_SEQUENTIAL_VOLUME 0x80 /* the reference's sequential volume
                                         walk (src/locate_pmmg.c:786-883 from
                                         the previous volume point's tet,
                                         src/interpmesh_pmmg.c:529,606): ties
                                         resolved by the reference's own path,
                                         a walk into a deleted tet returning
                                         the closest tet it visited.  Needs
                                         the new tets.  Default: the canonical
                                         (smallest-index) tet of a tie, and
                                         the exhaustive scan after a deleted
                                         tet                                  */
#define PMX_RUN_DEBUG_BARRIER_TIMEOUT 0x100 /* test hook: the fallback's grid
                                         barriers do not wait (the step must
                                         then fail, never return silently)   */
#define PMX_RUN_POINTMAP 0x200       /* every walk starts from its point's
                                         source vertex (pmx_upload_point_sources)
                                         as with the reference's USE_POINTMAP
                                         (PMMG_locate_setStart, src/locate_pmmg.c:
                                         931-986; src/interpmesh_pmmg.c:552-554,
                                         602-604): a surface point from the
                                         smallest tria holding the vertex, a
                                         volume point from the smallest valid
                                         tet holding it; element 1 when the
                                         source is outside 1..np of the
                                         background or no element holds it.  No
                                         hint grid is built.  Fails (0) without
                                         uploaded sources, and with either
                                         PMX_RUN_SEQUENTIAL_* flag              */
#define PMX_RUN_EAGER_DOWNLOAD   0x20 /* the step's fields start down into
                                         pinned staging as soon as it ends
                                         (overlapping the host work that
                                         follows pmx_run); pmx_download then
                                         only scatters them.  For callers that
                                         always download (the ParMmg seam
                                         sets it)                             */

/* Locate every uploaded new point in the background group and interpolate all
 * background solutions onto it.  Results stay on the device.  Asynchronous:
 * device-side failures (a fallback grid barrier that timed out) are reported
 * by the next pmx_synchronize / pmx_download, which then return 0. */
int pmx_run(pmx_ctx *ctx, const pmx_run_opts *opts);

/* Copy results to the host.  new_sols[s].m receives size*(npts) doubles in
 * point-list order (entries of REQ points and of failed tensor inversions are
 * left untouched).  elem/status/steps may be NULL.  Every host output call
 * takes the capacity its arrays were allocated for and returns 0 (nothing
 * written, pmx_last_error says why) when the device holds more: here
 * npts_cap rows -- size*npts_cap doubles per solution, npts_cap ints for
 * elem/status/steps -- with npts = last - first + 1 of the points view. */
int pmx_download(pmx_ctx *ctx, const pmx_sol_view *new_sols, int64_t npts_cap, int *elem,
                 int *status, int *steps);
/* After a pmx_run on ctx: nsol (>= 1, any number) further solutions of the
 * uploaded background, interpolated onto the points that step located, from
 * that step's elements.  old_sols[k].m: np+1 rows in Mmg layout; new_sols /
 * npts_cap as in pmx_download (rows the reference leaves alone are not
 * written).  Batched internally by PMX_MAX_SOLS.  0 + pmx_last_error: no step
 * yet, points or background uploaded since the step, null or mismatched views.
 * No walk is run: a volume point's barycentrics are recomputed from its
 * element and status, a surface point's were kept by the step.  The step's own
 * results (pmx_download) are not changed. */
int pmx_interp_more(pmx_ctx *ctx, int nsol, const pmx_sol_view *old_sols,
                    const pmx_sol_view *new_sols, int64_t npts_cap);
/* Per-point start element used by the device walk (debug/parity).  Volume
 * points' starts are recorded only by a pmx_run with PMX_RUN_RECORD_STARTS;
 * surface points' always.  cap: ints in start (>= npts). */
int pmx_download_starts(pmx_ctx *ctx, int *start, int64_t cap);
/* Per-point reference-style extras for boundary points: edge/vertex (-1
 * unset).  cap: ints in each array (>= npts). */
int pmx_download_border(pmx_ctx *ctx, int *edge, int *vertex, int64_t cap);
/* 1 when the context holds a step's results on its current points (a pmx_run
 * after the last pmx_upload_points), 0 otherwise -- e.g. a group whose
 * interpolation had nothing to locate (src/interpmesh_pmmg.c:497-512). */
int pmx_step_ready(pmx_ctx *ctx);
int pmx_locate_stats_get(pmx_ctx *ctx, pmx_locate_stats *st);
/* After a PMX_RUN_SEQUENTIAL_SURFACE step: the boundary points the reference
 * would locate (*nseq) and how many of them the device replayed one by one on
 * the reference's state (*nreplay; the others kept their speculative result:
 * same start tria as the reference, no shadow-wedge test on the way). */
int pmx_seq_surface_stats(pmx_ctx *ctx, int64_t *nseq, int64_t *nreplay);
/* The same for the volume points of a PMX_RUN_SEQUENTIAL_VOLUME step. */
int pmx_seq_volume_stats(pmx_ctx *ctx, int64_t *nseq, int64_t *nreplay);
/* Lane utilisation of the last step's walks (path 0 volume, 1 surface): a
 * wave iterates until its longest walk ends, so step_sum / lane_steps is the
 * fraction of lane-steps that did work.  Over the walk's per-wave records:
 * located points, their summed steps, 64 x the longest walk of each wave,
 * and the waves by their longest walk (entry 15: 15 steps or more). */
typedef struct {
  int64_t waves, located, step_sum, lane_steps;
  int64_t wave_max_hist[16];
} pmx_wave_stats;
int pmx_locate_wave_stats(pmx_ctx *ctx, int path, pmx_wave_stats *st);

/* Device pointers of the resident result buffers (for collectives / chaining):
 * which = 0 packed solutions [npts][S], 1 elem, 2 status. */
void *pmx_device_buffer(pmx_ctx *ctx, int which);
/* Device memory on the context's GPU for a C caller (zeroed): e.g. the
 * per-group partial records of the _device statistics functions. */
void *pmx_device_alloc(pmx_ctx *ctx, size_t bytes);
int pmx_device_free(pmx_ctx *ctx, void *p);
/* Copy bytes of device memory (e.g. such partial records) to the host, after
 * the context stream's earlier work; blocking. */
int pmx_device_download(pmx_ctx *ctx, void *host, const void *dev, size_t bytes);
/* and the other way (e.g. an empty partial record of a rank without a group) */
int pmx_device_upload(pmx_ctx *ctx, void *dev, const void *host, size_t bytes);
/* The first-incident-element maps of the last PMX_RUN_POINTMAP step's
 * background build: atomics[0] / atomics[1] = atomicMin operations the tet /
 * tria pass issued (a lane skips its atomic when the slot already holds a
 * smaller element), of 4 ne / 3 nt candidates. */
int pmx_pointmap_stats(pmx_ctx *ctx, int64_t atomics[2]);
/* Inspection: copy the volume hint grid of the last run to host (cap cells);
 * returns the number of cells (0 on error). */
int64_t pmx_debug_hint_grid(pmx_ctx *ctx, int *host, int64_t cap);
/* Inspection: a hint grid as the last pmx_run built it and its walks read it:
 * which = 0 the volume grid (cell -> a sampled tet whose centroid falls in
 * it), 1 the tria grid (cell -> the largest tria whose centroid falls in it);
 * 0 in an empty cell, cell (x, y, z) at x + dim[0] * (y + dim[1] * z).  desc
 * (may be NULL): the descriptor the kernels used -- cells per axis, the
 * fraction bits of the fixed-point vertex coordinates (volume grid only, 0
 * for the tria grid), the bounding box minimum and dim / extent per axis.
 * cells (NULL: the size query) receives every cell; cap: ints in cells.
 * Returns the number of cells, or 0 + pmx_last_error: no step on the current
 * background, more cells than cap, or the last step built no such grid (a
 * PMX_RUN_POINTMAP step builds neither; a step without surface points, or
 * with nothing to interpolate, no tria grid). */
typedef struct {
  int    dim[3];
  int    qf[3];
  double lo[3];
  double inv[3];
} pmx_grid_desc;
int64_t pmx_debug_grid(pmx_ctx *ctx, int which, pmx_grid_desc *desc, int *cells, int64_t cap);
/* Inspection: the process-wide number of live device and pinned allocations
 * the library owns (memory handed out by pmx_device_alloc is the caller's and
 * is not counted). */
int64_t pmx_debug_live_allocations(void);

/* ---- background topology on the device (the old-group
 * snapshot of src/grpsplit_pmmg.c:207-418) ------------------------------- */

/* Tet face adjacency, Mmg layout: adja[4*(k-1)+1+f] = 4*k'+f' (0 = boundary),
 * 4*ne+5 ints.  Replaces MMG3D_hashTetra's adjacency (called by ParMmg at
 * src/libparmmg1.c:272, src/distributemesh_pmmg.c:1185, src/metis_pmmg.c:756).
 * Tets with v[0] <= 0 are skipped.  Returns 1, or 0 on error / non-manifold
 * faces (pmx_last_error).  pmx_upload_background builds it the same way when
 * its mesh view has adja == NULL. */
int pmx_build_adja(pmx_ctx *ctx, int64_t ne, int64_t np, const int *tetra_v,
                   int64_t tetra_stride, int *adja);

/* Boundary trias (faces with adja 0) in (tet, face) order, vertices in
 * MMG5_idir order: tria[3*k+j], k = 1..nt (row 0 unused, maxnt rows at most);
 * and, if adjt != NULL, their edge adjacency adjt[3*(k-1)+1+e] = 3*k'+e'
 * (edge e = vertices (e+1)%3, (e+2)%3; 0 unless exactly 2 trias share it).
 * Replaces MMG5_chkBdryTria + MMG3D_hashTria on the snapshot
 * (src/grpsplit_pmmg.c:403-414).  Returns nt, or -1 on error. */
int64_t pmx_build_bdry(pmx_ctx *ctx, int64_t ne, int64_t np, const int *tetra_v,
                       int64_t tetra_stride, const int *adja, int *tria, int64_t maxnt,
                       int *adjt);

/* Device time (ms) of the last pmx_build_adja / pmx_build_bdry. */
double pmx_topo_ms(pmx_ctx *ctx);

/* Kernel timing of the last pmx_run with opts.timing != 0, in ms:
 * which = 0 hint build, 1 volume locate+interp, 2 surface locate+interp,
 * 3 exhaustive fallback, 4 total, 5 derived data, 6 the first-incident-element
 * maps of a PMX_RUN_POINTMAP step (0 when the step built none).
 * which = 7: the batch kernels of the last pmx_interp_more, summed over its
 * batches (always recorded; -1 before the first call).
 * which = 8: the device time of the last pmx_metis_graph, summed over its
 * kernels; 9 / 10 / 11 its count, scan and fill alone (-1 before the first
 * call).
 * which = 12 / 13: the labelling kernels / the replay and recolour kernels of
 * the last pmx_contiguity or pmx_fix_contiguity, summed (-1 before the first
 * call or after a refusal).
 * which = 14 / 15: the last pmx_split_groups / the last pmx_split_fetch after
 * it (-1 before the first, after a refusal of the plan and after a release).
 * which = 16 / 17 / 18: the last pmx_merge_groups / pmx_merge_fetch /
 * pmx_merge_adopt (each -1 before its first call, after a refusal of the plan
 * and after a release).
 * which = 19 / 20: the last pmx_moveifc_begin / the last pmx_moveifc_layer
 * (first to last device operation of the call; -1 before the first call, after
 * a refusal, after a release and once a background install dropped the state).
 * which = 21: the last pmx_split_adopt into ctx (first to last device
 * operation on ctx's stream; -1 before the first call and after a refused or
 * failed one).
 * which = 22 / 23: the kernels of the last pmx_check_reachability or
 * pmx_moveifc_reach, summed / those of the last pmx_moveifc_fix (-1 before the
 * first call and after a refusal; 23 also once the displacement is gone).  A
 * pmx_moveifc_fix sets 12 / 13 as pmx_fix_contiguity does.
 * which = 24: the last pmx_part_from_marks (first to last device operation of
 * the call; -1 before the first call, after a refusal and once the partition
 * is dropped or replaced by pmx_part_upload). */
double pmx_kernel_ms(pmx_ctx *ctx, int which);
/* Forget recorded kernel timings. */
int    pmx_timing_reset(pmx_ctx *ctx);

/* ---- drop-in mirrors of the reference seams ------------------------------ */
typedef struct {
  pmx_mesh_view    mesh;        /* new mesh (only points are read)            */
  pmx_points_view  points;      /* its vertices (first=1,last=np typically)   */
  pmx_sol_view    *met;         /* new metric (written), or NULL              */
  pmx_sol_view    *fields;      /* new fields (written), nsols entries        */
  int              nsols;
  double           hsiz;        /* mesh->info.hsiz                            */
  pmx_mesh_view    old_mesh;    /* background snapshot (old_listgrp)          */
  pmx_sol_view    *old_met;
  pmx_sol_view    *old_fields;
} pmx_group;

/* PMMG_interpMetricsAndFields (src/interpmesh_pmmg.c:663-741): loop on
 * groups; inputMet = parmesh->info.inputMet.  Returns 1 ok / 0 fail. */
int PMX_interpMetricsAndFields(pmx_ctx *ctx, int ngrp, pmx_group *grps,
                               const int *permNodGlob, int inputMet);

/* The same with one context per group: group g on ctxs[g] (caller-owned, all
 * on one device, e.g. kept across ParMmg iterations).  Every group's step is
 * enqueued before the first download, and each context keeps its group's new
 * points, new tets and results until its next upload -- so that
 * PMMG_tetraQual (src/libparmmg1.c:845) can run on them without a re-upload
 * (pmx_new_mesh_qual_synced).  Errors in pmx_last_error(ctxs[0]). */
int PMX_interpMetricsAndFields_groups(pmx_ctx *const *ctxs, int ngrp, pmx_group *grps,
                                      const int *permNodGlob, int inputMet);

/* The same with source vertices (ParMmg built with USE_POINTMAP): group g's
 * walks start from srcs[g] (pmx_upload_point_sources + PMX_RUN_POINTMAP).
 * srcs == NULL, or an entry with src == NULL: the hint grids for that group. */
typedef struct {
  const int *src;     /* &mesh->point[0].src */
  int64_t    stride;  /* sizeof(MMG5_Point)  */
} pmx_point_sources;
int PMX_interpMetricsAndFields_groups_src(pmx_ctx *const *ctxs, int ngrp, pmx_group *grps,
                                          const pmx_point_sources *srcs, const int *permNodGlob,
                                          int inputMet);

/* PMMG_copyMetricsAndFields_point (src/interpmesh_pmmg.c:432-446) on the
 * caller's host arrays (a host loop: nothing to do on the device). Old-point
 * tags are read through old_tag (uint16_t, stride bytes).  ctx may be NULL
 * (the reference calls it at src/libparmmg1.c:792, before the first
 * interpolation): errors then in pmx_last_error(NULL), per host thread. */
int PMX_copyMetricsAndFields_point(pmx_ctx *ctx, pmx_group *grp,
                                   const uint16_t *old_tag, int64_t old_tag_stride,
                                   const int *permNodGlob, int renum, int inputMet);

/* The same copy on device-resident data (PMMG_copySol_point, :311-358),
 * after a pmx_run: rows of the new points that the step did not write take
 * the background's values of its MG_REQ points (old ip -> new point
 * permNodGlob[ip], or ip; points-view numbering).  Equivalent to the
 * reference's copy before the interpolation, which then overwrites the rows
 * it writes.  Needs the background's point tags on the device (promoted, or
 * pmx_upload_point_tags); copy_metric: the metric too (inputMet and no
 * -hsiz, :378).  The copied rows count as written (pmx_download,
 * pmx_promote_background). */
int pmx_copy_required(pmx_ctx *ctx, const int *permNodGlob, int copy_metric);

/* ---- Medit files ---------------------------------
 * The wire format of the path's inputs and outputs: ParMmg reads/writes them
 * through Mmg (src/inout_pmmg.c:440-991 -> MMG3D_loadMesh / saveMesh /
 * loadSol / saveSol).  ASCII .mesh/.sol and binary .meshb/.solb (chosen by
 * the extension; binary versions 1-4 read, 2-4 written).  Arrays in Mmg's
 * layout (1-based, slot 0 untouched; tensors (11,12,13,22,23,33), converted
 * from/to Medit's (11,12,22,13,23,33)).  Keywords other than Vertices,
 * Tetrahedra, Triangles, RequiredVertices (mesh) and SolAtVertices (solution)
 * are skipped.  No context: errors in pmx_medit_last_error() (per thread). */
typedef struct {
  int64_t np, ne, nt, nreq;    /* vertices, tetrahedra, triangles, required vertices */
  int     dim, version;
} pmx_medit_info;
const char *pmx_medit_last_error(void);
int pmx_medit_mesh_info(const char *path, pmx_medit_info *info);
/* sized = the counts the arrays were allocated for (pmx_medit_mesh_info of
 * the same file): the read fails, writing nothing past them, if the file's
 * counts differ (changed file) or a keyword block appears twice.
 * xyz[3*(np+1)], tet[4*(ne+1)] required; vref[np+1], tetref[ne+1],
 * tria[3*(nt+1)], triaref[nt+1], req[nreq] may be NULL */
int pmx_medit_mesh_read(const char *path, const pmx_medit_info *sized, double *xyz, int *vref, int *tet,
                        int *tetref, int *tria, int *triaref, int *req);
int pmx_medit_mesh_write(const char *path, int64_t np, const double *xyz, const int *vref, int64_t ne,
                         const int *tet, const int *tetref, int64_t nt, const int *tria, const int *triaref,
                         int64_t nreq, const int *req);
/* solutions at vertices: types 1 scalar, 2 vector (3), 3 symmetric tensor (6) */
int pmx_medit_sol_info(const char *path, int64_t *np, int *nsol, int *types);
/* fields[s]: size(types[s])*(np+1); np, nsol, types = what the fields were
 * sized for (pmx_medit_sol_info): a different header fails the read */
int pmx_medit_sol_read(const char *path, int64_t np, int nsol, const int *types, double **fields);
int pmx_medit_sol_write(const char *path, int64_t np, int nsol, const int *types,
                        const double *const *fields);

/* ---- statistics ---------------------------------------------------------- */
/* Reference: PMMG_tetraQual / PMMG_qualhisto / PMMG_prilen (src/parmmg.h:564-566,
 * def src/quality_pmmg.c:156-733).  The per-element arithmetic is Mmg's,
 * restated (MMG5_caltet_iso / caltet33_ani, MMG5_lenEdg*; unpinned). */
#define PMX_INQUA  0          /* PMMG_INQUA : before the remesh                */
#define PMX_OUTQUA 1          /* PMMG_OUTQUA: after it (counts nrid, below)    */
#define PMX_LESQUA 2          /* mesh->info.optimLES: MMG3D_computeLESqua
                                 (src/quality_pmmg.c:221-224) -- not restated:
                                 the statistics calls refuse it (return 0)     */
#define PMX_TAG_GEO    2      /* MG_GEO  */
#define PMX_TAG_PARBDY 8192   /* MG_PARBDY */

/* Per-group partials as written to device memory by the *_device functions:
 * plain 8-byte fields, no padding (all-gathered as int64 words). */
typedef struct {
  double  avg, max, min;       /* alpha*q: SUM, max, min                     */
  int64_t iel, ne, np, good, med, nrid;
  int64_t his[5];
  int64_t iel_grp;             /* filled by the host fold                    */
} pmx_qual_part;               /* 15 x 8 B */
typedef struct {
  double  avlen, lmin, lmax;   /* avlen is the SUM over edges                */
  int64_t amin, bmin, amax, bmax, ned, nullEdge;
  int64_t hl[9];
} pmx_len_part;                /* 18 x 8 B */

/* ---- device residency across ParMmg iterations -------------------------
 * PMMG_update_oldGrps (src/libparmmg1.c:653) makes the group's current mesh
 * -- this iteration's new mesh with its interpolated metric and fields, and
 * the frozen points' copies (PMMG_copyMetricsAndFields_point, :792) -- the
 * next interpolation's background.  On the device that mesh already exists:
 * the new points, their tags and the step's results.  Replaces the
 * background upload (pmx_upload_background) of the next iteration when the
 * group was not renumbered in between (no load balancing of this group).
 *
 * pmx_upload_new_tets: the new mesh's tets (tetra_v as in pmx_mesh_view,
 * vertex indices in the last points view's numbering, !MG_EOK entries kept
 * as deleted) -- after pmx_upload_points, once per iteration (they also
 * serve pmx_new_mesh_qual).  A points view with tetra_v uploads them too
 * (packed and sent by the first pmx_run, the orphan marks made from them on
 * the device): no separate call needed then.
 *
 * pmx_promote_background: after a pmx_run on those points, the new points
 * (view first must be 1) become the background vertices 1..np, the step's
 * results its solutions (same list as the step), their tags its point tags.
 * Rows the step did not write (points not located, frozen, NUL, failed
 * interpolations) take the caller's values from sols[], in pmx_download's
 * point-list layout (entry 0 = point 1) -- the arrays pmx_download wrote into.  m: the new mesh --
 * np, ne (= the uploaded new tets), nt / tria_v / adjt / hausd of its
 * boundary trias (host, Mmg numbering), adja (optional: Mmg's mesh->adja,
 * else built on the device); point_c and tetra_v are not read.  Only the
 * trias (and adja when given) cross PCIe.  The new points and results are
 * consumed: upload the next iteration's points before the next pmx_run. */
int pmx_upload_new_tets(pmx_ctx *ctx, const int *tetra_v, int64_t tetra_stride, int64_t ne);
/* on: every points upload with new tets also builds, on a stream of its own
 * and while the step on those points runs, the next background's tet
 * records (face adjacency from the device-resident new tets); the following
 * pmx_promote_background (with m->adja = NULL) only swaps them in.  Off by
 * default: the drop-in path does not promote. */
int pmx_set_residency(pmx_ctx *ctx, int on);
int pmx_promote_background(pmx_ctx *ctx, const pmx_mesh_view *m, int nsol, const pmx_sol_view *sols);

/* Results (one group, or reduced over groups and ranks). */
typedef struct {
  int64_t ne, np;
  double  max, min, avg;       /* alpha*q, avg is the SUM (reference avg_cur) */
  int64_t iel;                 /* element realising min (1-based, in its group) */
  int64_t good, med;
  int64_t his[5];
  int64_t nrid;                /* OUTQUA: tets whose 4 vertices are ridge points */
  int     iel_grp, cpu;        /* group and rank of iel                      */
} pmx_qual_stats;

typedef struct {
  int64_t ned, nullEdge;
  double  avlen, lmin, lmax;   /* avlen is the SUM over edges                */
  int64_t amin, bmin, amax, bmax;
  int64_t hl[9];
  int     cpu_min, cpu_max;
} pmx_len_stats;

/* Point tags of the uploaded background (MMG5_Point.tag through a stride):
 * ridge points for the length loop's filter (src/quality_pmmg.c:509-517) and
 * OUTQUA's nrid.  NULL: no tags.  Kept until the next background upload. */
int pmx_upload_point_tags(pmx_ctx *ctx, const uint16_t *tag, int64_t tag_stride);

/* Quality of every background tet in the uploaded metric
 * (MMG3D_tetraQual(mesh, met, metRidTyp), src/quality_pmmg.c:726).  metRidTyp
 * 0 or 1: identical arithmetic for a size-1 metric (or none); with a size-6
 * metric 1 is MMG5_caltet_ani's ridge-aware mean (needs the point tags,
 * pmx_upload_point_tags: refused without them).  Result stays on the device;
 * qual may be NULL, else it holds qual_cap doubles (>= ne+1). */
int pmx_tetra_qual(pmx_ctx *ctx, int metRidTyp, double *qual, int64_t qual_cap);

/* PMMG_count_nodes_par (src/quality_pmmg.c:33-80) for the uploaded group:
 * the group's points in the internal node communicator (idx_ip[i] -> slot
 * idx_comm[i], nitem_grp entries) count when they claim their slot
 * (intvalues[slot] == 0 -> base; intvalues is the rank's array of nitem
 * slots, in/out, pre-marked by the caller for nodes a higher rank counts,
 * :196-209); every other point counts when a valid tet touches it.  The
 * count is the group's np in the next qualhisto partial. */
int pmx_count_nodes(pmx_ctx *ctx, const int *idx_ip, const int *idx_comm, int64_t nitem_grp,
                    int *intvalues, int64_t nitem, int base, int64_t *np);

/* The per-group part of PMMG_qualhisto (src/quality_pmmg.c:216-261) on the
 * uploaded group: opt PMX_INQUA / PMX_OUTQUA (PMX_LESQUA is refused); use_stored: the qualities of the
 * last pmx_tetra_qual.  Partial written to dev_result (pmx_qual_part, device
 * memory) on the context stream. */
int pmx_qualhisto_device(pmx_ctx *ctx, int opt, int use_stored, void *dev_result);
int pmx_qualhisto(pmx_ctx *ctx, int opt, pmx_qual_stats *st);

/* Parallel (interface) edges of the group for the distributed PMMG_prilen
 * (src/quality_pmmg.c:398-502): edge i joins a[i] -> b[i] (mesh->edge
 * orientation) and is owned by rank owner[i] (the lowest rank sharing it).
 * The owned edges are measured first, in list order, each once; the rank's
 * tet loop then measures every other edge -- the non-owned parallel edges
 * too, as the reference does (its warning at :585-586: interface edges are
 * counted by every rank holding them) unless exact_once is set. */
typedef struct {
  int64_t         n;
  const int      *a, *b, *owner;
  int             myrank;
  int             exact_once;
  /* the edge's tag from the parallel-edge hash (MMG5_hGet(&hpar, a, b, &ref,
   * &tag), :456): its MG_GEO bit is the isedg of MMG5_lenSurfEdg33_ani for a
   * tensor metric (:463).  NULL: 0 */
  const uint16_t *tag;
} pmx_par_edges;

/* Mmg's surface data of the uploaded group, read through strides as Mmg holds
 * it (1-based; pass &mesh->tetra[0].xt, sizeof(MMG5_Tetra);
 * &mesh->xtetra[0].tag[0], sizeof(MMG5_xTetra); &mesh->point[0].n[0] and
 * &mesh->point[0].xp, sizeof(MMG5_Point); &mesh->xpoint[0].n1[0] / .n2[0],
 * sizeof(MMG5_xPoint)).  The edge lengths in a tensor metric need it
 * (src/quality_pmmg.c:463,528,531 -> MMG5_lenedg33_ani / MMG5_lenedg_ani:
 * an edge tagged MG_BDY in its tet's xTetra is measured along the curved
 * surface from the point normals / ridge tangents, MMG5_lenSurfEdg33_ani /
 * MMG5_lenSurfEdg_ani, and with metRidTyp = 1 a ridge point's metric is rebuilt
 * per direction from its two xPoint normals, MMG5_buildridmet).  Never
 * uploaded after the background (or a NULL view): no tet has an xTetra and
 * every normal is 0 -- what Mmg holds for a mesh it never analysed.  Kept
 * until the next background upload; refused (0) if an index is out of range. */
typedef struct {
  int64_t         nxt, nxp;                     /* xTetra / xPoint counts   */
  const int      *tetra_xt;    int64_t tetra_stride;
  const uint16_t *xtetra_tag;  int64_t xtetra_stride;
  const double   *point_n;     const int *point_xp;  int64_t point_stride;
  const double   *xpoint_n1;   const double *xpoint_n2;  int64_t xpoint_stride;
} pmx_surface_view;
int pmx_upload_surface(pmx_ctx *ctx, const pmx_surface_view *sv);

/* PMMG_prilen on the uploaded group: centralized (par == NULL, the
 * MMG3D_computePrilen branch) or distributed (PMMG_computePrilen).  Tets whose
 * 4 vertices are ridge points (pmx_upload_point_tags) are skipped.  metRidTyp
 * (src/quality_pmmg.c:462-466,527-531): 0 or 1 for a size-1 metric (the same
 * lengths); with a size-6 metric 0 = classic storage (MMG5_lenedg33_ani /
 * MMG5_lenSurfEdg33_ani), 1 = Mmg's ridge storage (MMG5_lenedg_ani; the
 * parallel edges, as the reference writes them, MMG5_lenSurfEdg_iso on the
 * metric array read as isotropic: h = met->m[ip]), which needs the point tags
 * (refused without).  Surface edges use pmx_upload_surface's data. */
int pmx_prilen_device(pmx_ctx *ctx, int metRidTyp, const pmx_par_edges *par, void *dev_result);
int pmx_prilen(pmx_ctx *ctx, int metRidTyp, const pmx_par_edges *par, pmx_len_stats *st);

/* PMMG_graph_meshElts2metis (src/metis_pmmg.c:746-823) of the uploaded group:
 * the tets as Metis nodes.  xadj[0] = 0, xadj[k] = xadj[k-1] + the interior
 * faces of tet k; entries in (k, f) ascending order, adjncy[c] = jel - 1;
 * adjwgt[c] = max((int)PMMG_computeWgt(mesh, met, pt, f), 1) (:280-301): with
 * a metric min(1/exp(28 res/3), 1000000), res the sum over the face's edges
 * ia = MMG5_iarf[f][0..2] of (len <= 1 ? len - 1 : 1/len - 1), len =
 * MMG5_lenedg(mesh, met, ia, pt); without a metric 1000000.  The lengths are
 * pmx_prilen's: metRidTyp 0 or 1 for a size-1 metric (MMG5_lenedg_iso); a
 * size-6 metric takes MMG5_lenedg33_ani for 0 and MMG5_lenedg_ani for 1
 * (needs the point tags, refused without); tensor lengths of xTetra boundary
 * edges run along the surface (pmx_upload_surface).  MMG5_iarf, the lenedg
 * dispatch and the surface lengths are restated from Mmg, unpinned; exp is
 * the device library's, so a weight within an ulp of an integer may differ
 * by 1 from a glibc host's.
 * xadj: ne+1 ints.  adjncy / adjwgt: cap ints each (4*ne always suffices);
 * adjwgt NULL = no weights (the reference's *adjwgt == NULL: distribution
 * time and the last iteration).  adjncy NULL = count only (xadj and *nadjncy).
 * *nadjncy is set whenever the count ran.  Outputs are int32_t, the idx_t of
 * a default Metis build.  Returns 0 (pmx_last_error): no group uploaded,
 * 4*ne >= 2^31, a deleted tet (v[0] <= 0: the reference wants a packed mesh),
 * nadjncy > cap (*nadjncy set, no array written, the fill never launched),
 * metRidTyp = 1 with a tensor metric and no tags. */
int pmx_metis_graph(pmx_ctx *ctx, int metRidTyp, int32_t *xadj, int32_t *adjncy, int32_t *adjwgt,
                    int64_t cap, int64_t *nadjncy);
/* PMMG_computeWgt as a double for n listed faces of the uploaded group:
 * face[i] = 12*ie + 3*ifac (+ iloc, ignored), the encoding of
 * face2int_face_comm_index1 -- the interface-face weights of the group graph
 * (src/metis_pmmg.c:959) and PMMG_computeWgt_mesh (:242-266).  Returns 0 when
 * a face[i] is outside 12 .. 12*ne+11 or belongs to a deleted tet, and for
 * pmx_metis_graph's refusals. */
int pmx_face_weights(pmx_ctx *ctx, int metRidTyp, int64_t n, const int *face, double *wgt);

/* Partition contiguity of the uploaded (or promoted) group, on the tet
 * adjacency pmx_metis_graph reads.  Both calls refuse (return 0,
 * pmx_last_error): no group uploaded, 4*ne >= 2^31, a deleted tet (v[0] <= 0:
 * these callers run on packed meshes).  Host arrays are written only on
 * success.
 *
 * pmx_contiguity: the face-connected components of the graph restricted to
 * equal part values -- PMMG_check_part_contiguity (src/metis_pmmg.c:312-392)
 * for every part at once, and with part == NULL (one colour)
 * PMMG_check_grps_contiguity (:446-529) of the group.  part: ne entries, tet k
 * at k-1.  counts[p] (nparts entries, may be NULL): the components of part p
 * (the reference returns the last part's); values outside 0..nparts-1 are
 * labelled but counted nowhere.  label[k-1] (ne entries, may be NULL): the
 * smallest 1-based tet of k's component, the head the reference's ascending
 * scans find.  *ncomp: all components. */
int pmx_contiguity(pmx_ctx *ctx, const int32_t *part, int32_t nparts, int32_t *counts, int32_t *label,
                   int64_t *ncomp);

/* ncomp: components of the partition as given.  nmerged / nmerged_tets: lists
 * merged into a neighbouring colour and their tets.  ncannot: the reference's
 * "Cannot merge" warnings (a list with no neighbour outside).  counter: the
 * reference's counter.  rounds: hooking rounds over all labellings; relabels:
 * labellings after the first; replays: replay launches; replay_steps: tets
 * the replays dequeued. */
typedef struct {
  int64_t ncomp, nmerged, nmerged_tets, ncannot, counter;
  int64_t rounds, relabels, replays, replay_steps;
} pmx_contig_stats;

/* PMMG_fix_contiguity_split / _centralized (src/moveinterfaces_pmmg.c:377-523)
 * and PMMG_fix_contiguity after interface displacement (:525-611) on part
 * (in/out, ne entries): for each colour of colors[0..ncolors-1], in that
 * order, every face-connected piece but the largest is merged into the colour
 * of the first neighbouring tet its list meets -- the reference's lists, ties
 * and merge targets exactly.  colors NULL = 0..ncolors-1
 * (the split / centralized form); the interface-displacement form passes
 * colors[i] = nprocs*i + myrank, other values in part are merge targets only.
 * Duplicate colours and a NULL part are refused.  replay_steps: dequeues per
 * component per replay launch, 0 = the default (1024).  st may be NULL.
 * pmx_kernel_ms(ctx, 12 / 13): labelling / replay and recolour device time of
 * the last of these two calls. */
int pmx_fix_contiguity(pmx_ctx *ctx, int32_t *part, int32_t ncolors, const int32_t *colors,
                       int64_t replay_steps, pmx_contig_stats *st);

/* The uploaded (or promoted) group split by a partition: the new groups of
 * PMMG_split_eachGrp (src/grpsplit_pmmg.c:1267-1445) -- the tets, points,
 * adjacency and internal communicators PMMG_splitGrps_countTetPerGrp and
 * PMMG_splitGrps_fillGroup leave behind, the groups filled in the order
 * g = 0..ngrp-1 ("Group split").  Not produced: xTetra /
 * xPoint appends, the MG_PARBDY tags, PMMG_splitGrps_cleanMesh.
 * The tet records keep adja / 4 only: the neighbour's face is found as the one
 * that points back, so no two tets may share two faces.
 *
 * The old group's internal communicators (all optional: comm NULL, or counts
 * 0): face2int_face_comm_index1/2 (nface entries), node2int_node_comm_index1/2
 * (nnode entries), int_face_comm->nitem and int_node_comm->nitem on entry. */
typedef struct {
  int64_t nface, nnode;
  const int *face_index1, *face_index2, *node_index1, *node_index2;
  int64_t int_face_nitem, int_node_nitem;
} pmx_split_comm;
/* tets, points (poiPerGrp), face2int_face_comm and node2int_node_comm entries
 * of one new group */
typedef struct { int64_t ne, np, nface, nnode; } pmx_split_sizes;

/* The plan: everything is computed and kept on the device.  part: ne entries,
 * tet k at k-1, values 0..ngrp-1, every value used.  sizes: ngrp entries.
 * tet_new (ne ints, may be NULL): the local id of old tet k at k-1, the
 * reference's meshOld->tetra[k].flag.  *int_face_nitem / *int_node_nitem: the
 * internal communicators' nitem after the split.  Any ngrp <= ne works (no
 * table of ne x ngrp entries exists).  Returns 0 (pmx_last_error), the host
 * arrays untouched: no group uploaded; 4*ne >= 2^31; a deleted tet; part NULL;
 * ngrp < 1; a part value outside 0..ngrp-1; an empty part; 12*ne_g + 11 >= 2^31
 * for a group; an input face entry outside 12..12*ne+11 or on a face whose
 * adjacency is not 0; an input node outside 1..np.
 * pmx_kernel_ms(ctx, 14): the plan's device time (first to last device
 * operation of the call: the upload of part and the small table downloads
 * included, the tet_new download not); 15: the last fetch's (gather kernel
 * and copies); -1 before the first. */
int pmx_split_groups(pmx_ctx *ctx, const int32_t *part, int32_t ngrp, const pmx_split_comm *comm,
                     pmx_split_sizes *sizes, int *tet_new, int64_t *int_face_nitem, int64_t *int_node_nitem);

/* One new group's arrays, sized by the plan's sizes[g]; every pointer may be
 * NULL (not fetched):
 *   tet_old      ne ints: the old tet of local tet j at j-1 (tetra[j].flag)
 *   tetra_v      4*(ne+1) ints, Mmg layout: rows 1..ne written, local point ids
 *   adja         4*ne+5 ints, Mmg layout, all written: 4*j'+f' inside the
 *                group, 0 on the old boundary and on the new interface faces
 *   point_old    np ints: the old vertex of local point i at i-1
 *   face_index1/2  nface ints each: 12*j + 3*f + iploc and the position
 *   node_index1/2  nnode ints each: the local point and its value
 *   xyz          3*(np+1) doubles, rows 1..np written
 *   sols         nsol = 0 (none) or the number of uploaded solutions, of the
 *                uploaded sizes: m holds (np+1)*size doubles, rows 1..np written */
typedef struct {
  int *tet_old, *tetra_v, *adja, *point_old, *face_index1, *face_index2, *node_index1, *node_index2;
  double *xyz;
  int nsol;
  const pmx_sol_view *sols;
} pmx_split_out;
/* Returns 0, the arrays untouched: no plan (none made, released, or dropped by
 * a later pmx_upload_background / pmx_promote_background); g outside
 * 0..ngrp-1; solution views that do not match the uploaded ones.  The slices
 * are copied straight into the arrays, so a device error during the copies
 * (the only failure left after these checks) may leave them partly written. */
int pmx_split_fetch(pmx_ctx *ctx, int32_t g, const pmx_split_out *out);
/* Frees the plan's device memory (pmx_destroy does too). */
int pmx_split_release(pmx_ctx *ctx);

/* Group g of src's split plan becomes dst's uploaded group without crossing
 * PCIe: the new group of the last split of an iteration (PMMG_split_n2mGrps
 * with the Mmg target, src/loadbalancing_pmmg.c:135) as the next iteration's
 * background (PMMG_update_oldGrps, src/libparmmg1.c:653).  dst ends in the
 * state pmx_upload_background leaves, given the arrays pmx_split_fetch(src, g)
 * returns with every solution src carries, adja = NULL, the same imet, and
 *   surface = 1: nt, tria_v and adjt as MMG5_chkBdryTria + MMG3D_hashTria make
 *                them of the group (src/grpsplit_pmmg.c:400-414; what
 *                pmx_build_bdry returns for the fetched tets and adjacency:
 *                trias in (tet, face) order, vertices in MMG5_idir order, an
 *                edge adjacent only when exactly two trias share it), and hausd;
 *   surface = 0: nt = 0, as pmx_merge_adopt leaves it.
 * The library holds no tet ref: a face between tets of different ref is not a
 * tria (as for pmx_build_bdry).  dst carries no point tags (they change at a
 * split), and its own plans and derived data are dropped as by any upload.
 * src's plan and background are untouched: every group can be adopted in turn
 * into different contexts, and pmx_split_fetch still returns the same bytes.
 * dst's stream waits for src's; the call returns when dst's copies are done,
 * so src may release its plan right after.
 * Returns 0, pmx_last_error(dst) naming the cause and dst unchanged but for
 * its timing slot 21, which every call resets to -1 before its checks: a NULL
 * context (dst NULL: pmx_last_error(NULL)); dst == src; contexts on different
 * devices; no plan on src; g outside 0..ngrp-1; imet outside -1..nsol-1;
 * surface not 0 or 1; hausd not finite or negative.  Non-manifold tet faces
 * also return 0; dst then holds no background, as after a failed upload.
 * pmx_kernel_ms(dst, 21): the adopt's device time. */
int pmx_split_adopt(pmx_ctx *src, int32_t g, pmx_ctx *dst, int imet, int surface, double hausd);

/* The installed background's boundary trias as the device holds them, whether
 * uploaded, promoted or adopted -- a surface point's downloaded elem is a tria
 * index in this numbering.  Returns nt.  tria: 3*(nt+1) ints in Mmg layout,
 * rows 1..nt written (maxnt: the rows the array holds).  adjt (may be NULL):
 * 3*nt+4 ints, all written, adjt[3*(k-1)+1+e] = 3*k'+e' -- the device keeps
 * k' only; e' is the edge of k' that joins the same two vertices.  tria NULL:
 * the size query -- nt is returned, nothing is copied, maxnt and adjt are not
 * read (an adopt builds its trias on the device: ask before allocating).
 * Returns -1, the arrays untouched: no background installed, nt > maxnt. */
int64_t pmx_download_surface(pmx_ctx *ctx, int *tria, int64_t maxnt, int *adjt);

/* A rank's groups merged into one: PMMG_merge_grps (src/mergemesh_pmmg.c:
 * 967-1073) for packed groups, the first step of PMMG_split_n2mGrps
 * (src/grpsplit_pmmg.c:1736-1850) -- the merged points and tets in the
 * reference's order, the face and node slots of the internal communicators and
 * the merged communicators it rebuilds from the external ones (DESIGN.md
 * section 4, "Group merge").  Not produced: xPoint / xTetra copies, ref, tag,
 * qual (copy them through the maps), PMMG_updateTag.
 *
 * One group, in the vocabulary of pmx_split_out (a fetched group is a valid
 * input): point_c / tetra_v through byte strides, entries 1..np / 1..ne, as
 * pmx_mesh_view; sols: the call's nsol views, m holding (np+1)*size doubles;
 * node2int_node_comm_index1/2 (nnode entries: the local point, the position)
 * and face2int_face_comm_index1/2 (nface entries: 12*iel + 3*ifac + iploc,
 * the position). */
typedef struct {
  int64_t             np, ne;
  const double       *point_c;  int64_t point_stride;
  const int          *tetra_v;  int64_t tetra_stride;
  const pmx_sol_view *sols;
  int64_t             nnode, nface;
  const int          *node_index1, *node_index2, *face_index1, *face_index2;
} pmx_merge_group;
/* int_node_comm->nitem and int_face_comm->nitem on entry, and the rank's
 * external communicators as two CSR lists: next_node / next_face
 * communicators, node_off / face_off (next + 1 offsets, the first 0) into the
 * concatenated int_comm_index values node_items / face_items.  next = 0 (the
 * offsets and items may then be NULL) is the one-process case: both merged
 * communicators come out empty. */
typedef struct {
  int64_t        int_node_nitem, int_face_nitem;
  int32_t        next_node, next_face;
  const int64_t *node_off, *face_off;
  const int     *node_items, *face_items;
} pmx_merge_comm;
/* the merged group: points, tets, node2int_node_comm and face2int_face_comm
 * entries (= the two nitem after the merge) */
typedef struct { int64_t np, ne, nnode, nface; } pmx_merge_sizes;

/* The plan: the ngrp >= 1 groups are packed from the host views, uploaded and
 * merged on the device, where the result stays until pmx_merge_release, the
 * next pmx_merge_groups or pmx_destroy.  It neither needs, reads nor disturbs
 * an uploaded background; pmx_upload_background / pmx_promote_background do
 * not drop it.  comm NULL: both nitem 0, no external communicator.
 * Returns 0 (pmx_last_error), sizes untouched and no plan left: ngrp < 1; a
 * NULL view; a deleted tet (v[0] <= 0); a vertex outside 1..np_g; nsol outside
 * 0..PMX_MAX_SOLS, or a solution size that is not 1, 3 or 6 or differs between
 * groups; a node entry's point outside 1..np_g or its position outside
 * 0..int_node_nitem-1; a face entry outside 12..12*ne_g+11 or its position
 * outside 0..int_face_nitem-1; an external item out of range, or naming a slot
 * nothing filled (the reference asserts); a merged point that an external
 * node communicator holds twice, the first time as its first appearance (the
 * reference's poi_id_glo == nitem assert); the groups' points together, or the
 * merged np, >= 2^31 - 1; 12*ne + 11 >= 2^31.
 * pmx_kernel_ms(ctx, 16): the plan's device time (first to last device
 * operation of the call, the uploads and the small downloads included);
 * 17: the last pmx_merge_fetch; 18: the last pmx_merge_adopt; each -1 before
 * its first call, after a refused plan and after a release. */
int pmx_merge_groups(pmx_ctx *ctx, int32_t ngrp, const pmx_merge_group *groups, int nsol,
                     const pmx_merge_comm *comm, pmx_merge_sizes *sizes);

/* One source of a merge.  held == NULL: host views, exactly as
 * pmx_merge_groups reads g.  held != NULL: the points, tets and solutions are
 * those of the group that context holds as its background (uploaded, promoted,
 * split-adopted or merge-adopted) on ctx's device; of g only nnode, nface and
 * the four index arrays are read, in the held group's own numbering. */
typedef struct { pmx_ctx *held; pmx_merge_group g; } pmx_merge_source;

/* pmx_merge_groups with sources that contexts hold: both merges of
 * PMMG_split_n2mGrps (src/loadbalancing_pmmg.c:88,135) find their groups on
 * the device -- the remeshed groups promoted after the interpolation step, the
 * DISTR split's stayers one pmx_split_adopt away --, and only the groups MPI
 * delivered are host views.  Host and held sources mix in one call; ctx may be
 * a source, and a context may be named twice.  Of a held group nothing crosses
 * PCIe but its index arrays and a few control words: device kernels read its
 * vertex rows, connectivity and interleaved solution rows in place.
 *
 * A held group need not be packed (after MMG5_mmg3d1_delone the reference
 * packs the tets only, MMG5_paktet, src/libparmmg1.c:769).  A point that no
 * valid tet (v[0] > 0) of the group holds is dropped, as PMMG_merge_grps skips
 * !MG_VOK (src/mergemesh_pmmg.c:346,507); a deleted tet is dropped (:710); the
 * survivors keep their order, which is how PMMG_mark_packedTetra
 * (src/libparmmg1.c:102-113) and the points' tmp (:245-248) number a packed
 * group.  The result is pmx_merge_groups of the stably packed groups with the
 * ids mapped back: tet_old and point_old of the fetch are ids in the held
 * group's own numbering, pmx_merge_maps(g) is sized by its own np_g and ne_g
 * and holds 0 for a dropped point or tet, node_index1 / face_index1 are given
 * in its own numbering.  A deliberate difference: group 0 is compacted like
 * the others -- the reference fills group 0's holes through Mmg's free list
 * while it appends the other groups' entities, a numbering the library has
 * never reproduced; a packed group 0 gives the reference's numbering.  Host
 * sources keep pmx_merge_groups' contract: a deleted tet is refused, every
 * point is merged.
 *
 * The plan is an ordinary merge plan: pmx_merge_fetch, _maps, _adopt,
 * _release, pmx_moveifc_begin(tet_group = NULL) and the timing slots 16 to 18
 * work on it (slot 16: first to last device operation of this call).  ctx's
 * stream waits for each holder's; the call returns when its copies are done,
 * so a holder may be re-uploaded or destroyed right after.
 * Returns 0 (pmx_last_error(ctx), naming the group), sizes and every holder
 * untouched and no plan left: everything pmx_merge_groups refuses, for a held
 * group found by the device; sources NULL; a holder without a background, on
 * another device, with another nsol or other solution sizes than the call's
 * (those of the first source); a node or face entry that names a dropped point
 * or tet (the reference asserts, :59, :622); a holder whose points are all
 * dropped. */
int pmx_merge_groups_from(pmx_ctx *ctx, int32_t ngrp, const pmx_merge_source *sources, int nsol,
                          const pmx_merge_comm *comm, pmx_merge_sizes *sizes);

/* The merged group's arrays, sized by the plan's sizes; every pointer may be
 * NULL (not fetched):
 *   tetra_v        4*(ne+1) ints, Mmg layout: rows 1..ne written
 *   tet_group      ne ints: the group merged tet j came from, at j-1 (what
 *                  PMMG_set_color_tetra leaves in mark)
 *   tet_old        ne ints: its local id in that group (a held source of
 *                  pmx_merge_groups_from: in the held group's own numbering;
 *                  point_old likewise)
 *   point_group    np ints: the group whose copy created merged point i, at i-1
 *   point_old      np ints: that copy's local id
 *   xyz            3*(np+1) doubles, rows 1..np written: the creating copy's
 *   sols           nsol = 0 (none) or the plan's, of the plan's sizes: m holds
 *                  (np+1)*size doubles, rows 1..np written
 *   node_index1/2  nnode ints each: the merged point and its position
 *   face_index1/2  nface ints each: 12*ie + 3*ifac + iploc and the position
 *   ext_node_items / ext_face_items  the external communicators' rewritten
 *                  int_comm_index, in the input's CSR layout
 * Returns 0, the arrays untouched: no plan; solution views that do not match
 * the plan's.  A device error during the copies may leave them partly written. */
typedef struct {
  int *tetra_v, *tet_group, *tet_old, *point_group, *point_old;
  double *xyz;
  int nsol;
  const pmx_sol_view *sols;
  int *node_index1, *node_index2, *face_index1, *face_index2, *ext_node_items, *ext_face_items;
} pmx_merge_out;
int pmx_merge_fetch(pmx_ctx *ctx, const pmx_merge_out *out);

/* Group g's local-to-merged maps: point_new (np_g ints, local point k at k-1:
 * meshJ->point[k].tmp) and tet_new (ne_g ints: tetra[k].flag); either may be
 * NULL.  After pmx_merge_groups_from np_g and ne_g are the source's own sizes
 * (a held group's, unused points and deleted tets counted: their entries are
 * 0).  Returns 0, the arrays untouched: no plan; g outside 0..ngrp-1. */
int pmx_merge_maps(pmx_ctx *ctx, int32_t g, int *point_new, int *tet_new);

/* The merged group becomes the context's uploaded group without crossing
 * PCIe: the context ends in the state pmx_upload_background of the fetched
 * arrays with adja = NULL, nt = 0 and the same imet leaves (tet records by
 * device face matching -- the reference's MMG3D_hashTetra after the merge,
 * src/grpsplit_pmmg.c:1815-1821 --, xyz, the interleaved solutions, grids and
 * hint samples; the same flags invalidated, a split plan included).  The
 * merge plan survives and stays fetchable.  Returns 0: no plan; imet outside
 * -1..nsol-1; 4*ne >= 2^31; non-manifold faces (the context then holds no
 * background, as after a failed upload). */
int pmx_merge_adopt(pmx_ctx *ctx, int imet);
/* Frees the plan's device memory (pmx_destroy does too). */
int pmx_merge_release(pmx_ctx *ctx);

/* Interface displacement of the uploaded (or adopted) group: the steps of the
 * reference's default repartitioning mode between the merge and
 * PMMG_fix_contiguity -- PMMG_set_color_tetra, PMMG_mark_interfacePoints and
 * the layers of PMMG_part_moveInterfaces (src/moveinterfaces_pmmg.c:119-134,
 * 1052-1090, 1306-1440) --, and PMMG_part_getInterfaces (:1150-1212) after the
 * fix ("Interface displacement").  The marks, the
 * per-point state and negrp equal the reference's sequential loops, blocked
 * layers included.  The state lives on the device until pmx_moveifc_release,
 * the next pmx_moveifc_begin or pmx_destroy; pmx_upload_background,
 * pmx_promote_background and pmx_merge_adopt drop it, as they drop a split plan.
 *
 * The priority map: a colour is nprocs*igrp + iproc, its weight
 * mapgrp[igrp + displsgrp[iproc]] (the old group's tet count before the merge,
 * gathered over the ranks); the lighter colour wins, the first met among equal
 * ones.  displsgrp: nprocs + 1 entries from 0; nold_grp: this rank's old
 * groups, displsgrp[myrank + 1] - displsgrp[myrank]. */
typedef struct {
  int32_t nprocs, myrank, nold_grp;
  const int *displsgrp, *mapgrp;
} pmx_moveifc_map;

/* One layer.  front: front points walked; touched: front points a neighbouring
 * ball recoloured towards (the side fronts); recolor: recolourings, a tet
 * that changes twice counts twice; next: points of the following front;
 * blocked: 1 when a group would have passed below nemin, so that the layer
 * ran as the reference's sequential loop on one lane; blocks: balls that loop
 * abandoned; maxball: the longest ball walked to its end; seq_launches:
 * launches of the sequential loop; overflow_ip: the point whose ball
 * overflowed (0: none). */
typedef struct {
  int64_t front, touched, recolor, next, blocked, blocks, maxball, seq_launches, overflow_ip;
} pmx_moveifc_stats;

/* tet_group: ne ints, the old group of tet k at k-1 (pmx_merge_out.tet_group);
 * NULL: the live merge plan's, read on the device (after pmx_merge_adopt).
 * The marks become nprocs*tet_group + myrank, every point takes the lightest
 * colour around it and the slot 4*tet + iloc it met it first at, the front is
 * the points that met a lighter colour after their first slot, negrp[g] =
 * mapgrp of the local group g and nemin[g] = min(6, negrp[g]/2 + 1).
 * *nfront (may be NULL): the front points.  Returns 0 (pmx_last_error),
 * *nfront untouched: no group uploaded; 4*ne >= 2^31; a deleted tet; a
 * tet_group value outside 0..nold_grp-1; a colour that occurs with mapgrp <= 0
 * (the reference asserts); displsgrp not ascending from 0 or disagreeing with
 * nold_grp; tet_group NULL without a merge plan of ne tets.
 * pmx_kernel_ms(ctx, 19): its device time. */
int pmx_moveifc_begin(pmx_ctx *ctx, const int32_t *tet_group, const pmx_moveifc_map *map, int64_t *nfront);

/* The two ends of the node-communicator exchange before a layer
 * (src/moveinterfaces_pmmg.c:1369-1376, 1406-1413) for the points ip[0..n-1]
 * (node2int_node_comm_index1): get delivers their colours (tmp), set writes
 * the reduced ones and makes every listed point front, whether its colour
 * changed or not.  A point is expected once; listed twice it keeps the colour
 * of its last entry, as the reference's loop would.  The exchange and its
 * reduction stay with the caller.
 * Refused, nothing written: no displacement begun; a point outside 1..np; for
 * set a colour of no group or of one with mapgrp <= 0. */
int pmx_moveifc_get_colors(pmx_ctx *ctx, int64_t n, const int *ip, int *color);
int pmx_moveifc_set_colors(pmx_ctx *ctx, int64_t n, const int *ip, const int *color);

/* One pass of src/moveinterfaces_pmmg.c:1415-1438: the balls of the front
 * points in ascending order, the side fronts, the next front.  seq_steps:
 * steps (ball tets visited) per launch of the sequential loop, 0 = the default
 * (65536).  st may be
 * NULL.  A deliberate difference: a ball of more than MMG3D_LMAX - 2 = 10238
 * tets makes the reference leave the layer half-way; here the call returns 0,
 * names the point (pmx_last_error, st->overflow_ip) and the state stays as at
 * the layer's start, so that the caller can take the CPU path.
 * pmx_kernel_ms(ctx, 20): its device time. */
int pmx_moveifc_layer(pmx_ctx *ctx, int64_t seq_steps, pmx_moveifc_stats *st);

/* The marks (ne ints, tet k at k-1): the part pmx_fix_contiguity takes in its
 * interface-displacement form. */
int pmx_moveifc_marks(pmx_ctx *ctx, int32_t *mark);
/* The per-point state (np ints each, point i at i-1; any may be NULL): the
 * colour, the slot 4*tet + iloc (-1 both for a point in no tet) and 1 on the
 * front. */
int pmx_moveifc_points(pmx_ctx *ctx, int *tmp, int *s, int *front);
/* negrp and nemin of the local groups (nold_grp ints each; either may be NULL). */
int pmx_moveifc_groups(pmx_ctx *ctx, int *negrp, int *nemin);

/* PMMG_part_getInterfaces: the partition the marks stand for.  mark: ne ints
 * (after pmx_fix_contiguity), NULL = the device's.  PMX_GRPSPL_MMG_TARGET:
 * part = mark / nprocs, *ngrp = nold_grp; a mark of another rank is refused
 * (the reference asserts).  PMX_GRPSPL_DISTR_TARGET: the used colours numbered
 * from 0, ranks visited from myrank round; ngrps_all: the old groups of every
 * rank (nprocs ints, NULL = the map's).  part: ne ints, written on success. */
#define PMX_GRPSPL_DISTR_TARGET 1
#define PMX_GRPSPL_MMG_TARGET 2
int pmx_moveifc_part(pmx_ctx *ctx, const int32_t *mark, int target, const int *ngrps_all, int32_t *part,
                     int32_t *ngrp);
/* Frees the displacement's device memory (pmx_destroy does too). */
int pmx_moveifc_release(pmx_ctx *ctx);

/* ---- reachability (PMMG_check_reachability, src/moveinterfaces_pmmg.c:627-811) ----
 * The call that ends PMMG_part_moveInterfaces after PMMG_fix_contiguity: a
 * piece of another rank's colour must touch that rank through a face of the
 * face communicator, or it joins a neighbouring piece.  The exchange of the
 * colours (step 1, :651-716) stays with the caller; pmx_reach_face_marks
 * gives what it sends.  The tets' flags the reference carries over from the
 * fix are a function of the fixed marks: a tet is flagged exactly when its
 * mark is one of the rank's colours ("Reachability").
 * Every call below returns 0 without touching its outputs, *counter or the
 * device's marks when: no group is uploaded; 4 ne >= 2^31; nface < 0 or an
 * array is NULL with nface > 0; an entry's tet face_index1[i] / 12 lies
 * outside 1..ne; a colour is listed twice; counter is NULL. */
typedef struct {
  int64_t nseeds, nreached, nreached_tets;     /* step 2: entries that seeded (tet unflagged on entry, colour
                                                  as received), lists flagged, their tets */
  int64_t nunreached, nmerged, nmerged_tets;   /* step 3: lists met, merged, tets recoloured (a tet counts each time) */
  int64_t nrescanned, ncannot, counter;        /* merges into an unflagged list; lists with no neighbour outside;
                                                  *counter at the end */
  int64_t rounds, relabels, replays, replay_steps;   /* rounds of step 3 (0: nothing was left), labellings after
                                                  the first, replay launches, tets dequeued */
} pmx_reach_stats;

/* out[i] = mark[face_index1[i] / 12], i < nface: what the caller puts into
 * intvalues before the exchange (:664-670).  mark: ne ints, tet k at k-1;
 * NULL = the live displacement's marks on the device (refused without one). */
int pmx_reach_face_marks(pmx_ctx *ctx, const int32_t *mark, int64_t nface, const int *face_index1, int32_t *out);

/* Steps 2 and 3 on mark (ne ints, in/out), after pmx_fix_contiguity with the
 * same colours (NULL = 0..ncolors-1).  color_in[i]: the colour received for
 * entry i after the discard of :708-716, -1 (PMMG_UNSET) = none.  Step 2:
 * every unflagged piece that holds the tet of an entry whose colour is the
 * tet's mark is flagged.  Step 3: the tets are scanned upwards; at an
 * unflagged tet its piece -- the unflagged tets of its mark, breadth-first,
 * faces 0..3 -- takes mark and flag of its first neighbour outside the list,
 * met in list order; without one it stays.  A piece that joined an unflagged
 * neighbour is met again further up.  *counter: in, the fix's counter; out, the
 * reference's (ne on a connected mesh).  replay_steps: dequeues per launch of
 * the list replay, 0 = pmx_fix_contiguity's default.  st may be NULL.
 * pmx_kernel_ms(ctx, 22): its device time. */
int pmx_check_reachability(pmx_ctx *ctx, int32_t *mark, int32_t ncolors, const int32_t *colors, int64_t nface,
                           const int *face_index1, const int32_t *color_in, int64_t *counter, int64_t replay_steps,
                           pmx_reach_stats *st);

/* The same two calls on the live displacement's marks, in place on the device:
 * nothing of size ne crosses PCIe, and pmx_moveifc_marks and
 * pmx_moveifc_part(mark = NULL) return the result.  pmx_moveifc_fix is
 * pmx_fix_contiguity with the colours nprocs * i + myrank, i < nold_grp;
 * pmx_moveifc_reach carries its counter on (st->counter) and is refused
 * without a pmx_moveifc_fix since the last layer, set_colors or reach.  Both
 * are refused without a live displacement.  The marks change only when the
 * call succeeds.  pmx_kernel_ms(ctx, 23) / (ctx, 22): their device times. */
int pmx_moveifc_fix(pmx_ctx *ctx, int64_t replay_steps, pmx_contig_stats *st);
int pmx_moveifc_reach(pmx_ctx *ctx, int64_t nface, const int *face_index1, const int32_t *color_in,
                      int64_t replay_steps, pmx_reach_stats *st);

/* ---- the partition on the device, from the marks (or Metis) to the split ----
 * The context holds at most one partition of the uploaded group: ne ints in
 * 0..ngrp-1 on the device.  pmx_part_from_marks or pmx_part_upload fills it,
 * pmx_part_fix repairs it, pmx_split_groups_part splits by it; nothing of size
 * ne crosses PCIe on the way.  A background upload, a promotion, an adoption
 * (pmx_split_adopt into this context, pmx_merge_adopt) and pmx_destroy drop
 * it, as they drop the split plan and the displacement; pmx_moveifc_release
 * does not.  A refused call leaves its outputs and the held partition as they
 * were.
 *
 * pmx_part_from_marks: PMMG_part_getInterfaces on the live displacement's
 * marks (refused without one); targets, ngrps_all and refusals as
 * pmx_moveifc_part(mark = NULL).  *ngrp (may be NULL): the groups.
 * group_mark (may be NULL, *ngrp ints -- at most nold_grp under the MMG
 * target, the sum of ngrps_all under DISTR): the mark every tet of group g
 * carries, nprocs * g + myrank under the MMG target; group_mark[g] % nprocs is
 * the owner PMMG_part_getProcs reads off the group's first tet.
 * pmx_kernel_ms(ctx, 24): its device time. */
int pmx_part_from_marks(pmx_ctx *ctx, int target, const int *ngrps_all, int32_t *ngrp, int32_t *group_mark);
/* A host partition (Metis's; ne ints, tet k at k-1) becomes the context's.
 * ngrp < 1 or a value outside 0..ngrp-1 (checked on the device) is refused. */
int pmx_part_upload(pmx_ctx *ctx, const int32_t *part, int32_t ngrp);
/* The held partition: part (ne ints) and *ngrp, either may be NULL. */
int pmx_part_download(pmx_ctx *ctx, int32_t *part, int32_t *ngrp);
/* PMMG_fix_contiguity_split in place: pmx_fix_contiguity with the colours
 * 0..ngrp-1.  Sets pmx_kernel_ms(ctx, 12 / 13) as that call does. */
int pmx_part_fix(pmx_ctx *ctx, int64_t replay_steps, pmx_contig_stats *st);
/* pmx_split_groups by the held partition (sizes: its ngrp entries): the same
 * refusals -- "no partition" for "part is NULL" --, the same plan;
 * pmx_split_fetch and pmx_split_adopt follow. */
int pmx_split_groups_part(pmx_ctx *ctx, const pmx_split_comm *comm, pmx_split_sizes *sizes, int *tet_new,
                          int64_t *int_face_nitem, int64_t *int_node_nitem);
/* Frees the partition's device memory (pmx_destroy does too). */
int pmx_part_release(pmx_ctx *ctx);

/* PMMG_tetraQual(parmesh, metRidTyp) on the NEW mesh right after the
 * interpolation (src/libparmmg1.c:845, metRidTyp = 1; a size-6 metric
 * takes MMG5_caltet_ani's ridge-aware mean as in pmx_tetra_qual): the new tets (1-based records through a stride,
 * vertex indices in the last points view's numbering) are uploaded as by
 * pmx_upload_new_tets -- or tetra_v = NULL: the ones already uploaded; the
 * coordinates and the interpolated metric are the step's device-resident
 * points and results.  qual (host, qual_cap doubles >= ne+1) and/or
 * dev_result (the qualhisto partial of the new mesh, opt as above; np = the
 * points) may be NULL.  Needs a pmx_run on those points. */
int pmx_new_mesh_qual(pmx_ctx *ctx, const int *tetra_v, int64_t tetra_stride, int64_t ne, int opt,
                      int metRidTyp, double *qual, int64_t qual_cap, void *dev_result);

/* PMMG_tetraQual(parmesh, metRidTyp) on the new mesh of the last step
 * (src/libparmmg1.c:845, right after PMMG_interpMetricsAndFields) in the
 * caller's metric array met (Mmg layout, the points view's numbering; NULL
 * or met->m NULL: no metric): the device already holds the new points, the
 * new tets (the points view must have carried them) and the interpolated
 * metric; only the rows the step did not write -- frozen points the caller
 * filled (PMMG_copyMetricsAndFields_point), failed tensor inversions -- are
 * sent, or the whole array when the step interpolated no metric (-hsiz, Mmg's
 * own metric).  dev_result as in pmx_new_mesh_qual.  qual: the qualities of
 * tets 1..ne through qual_stride bytes -- 0 or 8: a dense array of ne+1
 * doubles, every entry written (deleted tets 0, qual[0] = 0); any larger
 * stride: an AoS field such as &mesh->tetra[0].qual with sizeof(MMG5_Tetra),
 * written for the valid tets only (MMG3D_tetraQual skips !MG_EOK) -- straight
 * from pinned staging, no intermediate array.  qual_cap: the records the
 * array holds (entries 0 .. qual_cap-1; >= ne+1, e.g. mesh->nemax+1). */
int pmx_new_mesh_qual_synced(pmx_ctx *ctx, const pmx_sol_view *met, int opt, int metRidTyp, double *qual,
                             int64_t qual_stride, int64_t qual_cap, void *dev_result);

/* The reduction across groups and ranks (the reference's MPI_Reduce with its
 * custom operators, src/quality_pmmg.c:82-144, :265-307, :661-676), as host
 * folds in (rank, group) order -- deterministic; ties go to the first:
 *   pmx_qual_fold: parts[i] of rank[i] (nondecreasing; NULL = one group per
 *     rank), groups folded as PMMG_qualhisto's loop, then ranks;
 *   pmx_len_fold:  one part per rank, with the reference's operator
 *     (a smaller lmin also takes the other rank's amax/bmax, :125-131). */
int pmx_qual_fold(const pmx_qual_part *parts, const int *rank, int n, pmx_qual_stats *out);
int pmx_len_fold(const pmx_len_part *parts, int n, pmx_len_stats *out);

/* RCCL: one all-gather of the ranks' device partials on the context stream,
 * then the fold.  comm is an ncclComm_t (void *): pmx_comm_unique_id on one
 * rank (broadcast the bytes, e.g. MPI_Bcast on parmesh->comm), pmx_comm_init
 * on every rank. */
int pmx_comm_unique_id(char *id, int len);
int pmx_comm_init(pmx_ctx *ctx, void **comm, int nranks, const char *id, int rank);
int pmx_comm_destroy(void *comm);
/* dev_parts: this rank's ngrp group partials (pmx_qual_part, contiguous in
 * device memory), merged on the host before the all-gather. */
int pmx_qualhisto_allreduce(pmx_ctx *ctx, void *comm, int nranks, const void *dev_parts, int ngrp,
                            pmx_qual_stats *out);
int pmx_prilen_allreduce(pmx_ctx *ctx, void *comm, int nranks, const void *dev_part,
                         pmx_len_stats *out);

#ifdef __cplusplus
}
#endif
#endif
