"""Host-side mirror of ParMmg's transfer interface, over the C ABI.

Names and argument meaning follow the reference:

* :meth:`Transfer.interp_metrics_and_fields` -- ``PMMG_interpMetricsAndFields``
  (reference src/interpmesh_pmmg.c:663-741), one call per remesh iteration,
  groups are independent.
* :meth:`Transfer.copy_metrics_and_fields_point` --
  ``PMMG_copyMetricsAndFields_point`` (src/interpmesh_pmmg.c:432-446).
* :meth:`Transfer.tetra_qual`, :meth:`Transfer.qualhisto`,
  :meth:`Transfer.prilen` -- ``PMMG_tetraQual`` / ``PMMG_qualhisto`` /
  ``PMMG_prilen`` (src/quality_pmmg.c).
* :meth:`Transfer.metis_graph`, :meth:`Transfer.face_weights` --
  ``PMMG_graph_meshElts2metis`` / ``PMMG_computeWgt`` (src/metis_pmmg.c).
* :meth:`Transfer.contiguity`, :meth:`Transfer.fix_contiguity` --
  ``PMMG_check_grps_contiguity`` / ``PMMG_check_part_contiguity``
  (src/metis_pmmg.c) and ``PMMG_fix_contiguity*`` (src/moveinterfaces_pmmg.c).
* :meth:`Transfer.split_groups`, :meth:`Transfer.split_fetch`,
  :meth:`Transfer.split_release` -- the new groups of ``PMMG_split_eachGrp``
  (src/grpsplit_pmmg.c); :meth:`Transfer.split_adopt` makes one of them
  another context's background on the device (``PMMG_update_oldGrps``,
  src/libparmmg1.c:653), :meth:`Transfer.download_surface` reads a
  background's boundary trias back.
* :meth:`Transfer.merge_groups`, :meth:`Transfer.merge_groups_from`, :meth:`Transfer.merge_fetch`,
  :meth:`Transfer.merge_maps`, :meth:`Transfer.merge_adopt`,
  :meth:`Transfer.merge_release` -- ``PMMG_merge_grps``
  (src/mergemesh_pmmg.c), the merged group kept on the device.

Errors follow the reference's 1/0 convention at the C ABI and surface here as
``RuntimeError`` with ``pmx_last_error``.  Everything runs on the GPU; there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _native as N
from .mesh import Mesh


def _dp(a):
    return a.ctypes.data_as(N.dptr) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(N.iptr) if a is not None else None


def _shift(a, rec: int, ctype):
    """Pointer to record -1 of a 0-based array: a 1-based view (the library
    only dereferences records first..last >= 1)."""
    return C.cast(C.c_void_p(a.ctypes.data - rec), C.POINTER(ctype))


def _tets_1based(tets) -> np.ndarray:
    """0-based new tets (v[0] < 0: deleted) -> Mmg's 1-based records (v[0] = 0)."""
    tv = np.ascontiguousarray(tets, np.int32) + 1
    tv[tv[:, 0] < 0, 0] = 0
    tv[0] = 0
    return tv


def mesh_view(m: Mesh) -> N.MeshView:
    v = N.MeshView()
    v.np, v.ne, v.nt = m.np, m.ne, m.nt
    v.point_c = _dp(m.xyz)
    v.point_stride = 3 * 8
    v.tetra_v = _ip(m.tet)
    v.tetra_stride = 4 * 4
    v.adja = _ip(m.adja)
    v.tria_v = _ip(m.tria) if m.nt > 0 else None
    v.tria_stride = 3 * 4
    v.adjt = _ip(m.adjt) if m.nt > 0 else None
    v.hausd = m.hausd
    return v


@dataclasses.dataclass
class Result:
    sols: list            # per solution: (npts, size) arrays
    elem: np.ndarray      # located tet (volume) / tria (surface), 1-based
    status: np.ndarray    # 1 found, -1 found by exhaustive search, 0 closest
    steps: np.ndarray


class Transfer:
    """One device context (one GPU).  ``device`` = rank % ndev in ParMmg terms."""

    def __init__(self, device: int = 0):
        self._peer = None     # second context of interp_metrics_and_fields with sources
        self.device = device
        self.lib = N.load()
        self.ctx = self.lib.pmx_create(device)
        if not self.ctx:
            raise RuntimeError("pmx_create failed (no HIP device visible)")
        self._keep = []
        self.sizes: list[int] = []
        self.bg_np = 0        # vertices of the uploaded background
        self.bg_ne = 0        # ... and its tets
        self.bg_nt = 0        # ... and its trias
        self.npts = 0
        self.n_new_tets = 0

    def close(self):
        if self._peer is not None:
            self._peer.close()
            self._peer = None
        if self.ctx:
            self.lib.pmx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r: int, what: str):
        if not r:
            raise RuntimeError(f"{what}: {self.lib.pmx_last_error(self.ctx).decode()}")

    def device_info(self) -> str:
        buf = C.create_string_buffer(256)
        self._chk(self.lib.pmx_device_info(self.ctx, buf, 256), "pmx_device_info")
        return buf.value.decode()

    def set_stream(self, stream_ptr: int | None):
        self._chk(self.lib.pmx_set_stream(self.ctx, C.c_void_p(stream_ptr or 0)), "pmx_set_stream")

    def synchronize(self):
        self._chk(self.lib.pmx_synchronize(self.ctx), "pmx_synchronize")

    # ---- device-resident interface ------------------------------------------
    def upload_background(self, m: Mesh, sols: list[np.ndarray], imet: int = 0, adja: bool = True):
        """sols: (np+1, size) arrays in Mmg layout; imet: index of the metric or -1.
        adja=False: Mmg's adjacency is not sent; the device rebuilds it from the
        connectivity (16 B/tet less over PCIe, face matching overlapped with
        the rest of the upload)."""
        arr = [np.ascontiguousarray(s, np.float64) for s in sols]
        views = (N.SolView * max(len(arr), 1))()
        for i, a in enumerate(arr):
            views[i].size = a.shape[1] if a.ndim == 2 else 1
            views[i].m = _dp(a)
        mv = mesh_view(m)
        if not adja:
            mv.adja = None
        self._chk(self.lib.pmx_upload_background(self.ctx, C.byref(mv), len(arr), views,
                                                 imet if arr else -1), "pmx_upload_background")
        self.sizes = [v.size for v in views[: len(arr)]]
        self.bg_np = m.np
        self.bg_ne = m.ne
        self.bg_nt = m.nt

    def copy_required(self, perm: np.ndarray | None = None, copy_metric: bool = True):
        """pmx_copy_required: frozen (MG_REQ) background points' values into the
        unwritten rows of the last step's results; perm: (np+1,) permNodGlob
        (1-based new point of background vertex ip)."""
        pp = None if perm is None else np.ascontiguousarray(perm, np.int32)
        self._chk(self.lib.pmx_copy_required(self.ctx, _ip(pp), int(copy_metric)), "pmx_copy_required")

    def set_residency(self, on: bool = True):
        self._chk(self.lib.pmx_set_residency(self.ctx, int(on)), "pmx_set_residency")

    def upload_points(self, xyz: np.ndarray, tags: np.ndarray | None = None,
                      tets: np.ndarray | None = None, tets_mmg: np.ndarray | None = None):
        """xyz: (n, 3) new points (0-based list); tags: MMG5_Point.tag values;
        tets: optional (ne+1, 4) new tets with 0-based point indices in rows
        1..ne -- only points of valid tets (v[0] >= 0 here) are located.
        The C view is Mmg's 1-based one (points 1..n, a tet valid when
        v[0] > 0), so the pointers are shifted by one record.  tets_mmg: the
        same tets already in that layout (1-based, v[0] = 0 deleted; passed
        as is, as a C caller would)."""
        xyz = np.ascontiguousarray(xyz, np.float64)
        pv = N.PointsView()
        pv.first, pv.last = 1, xyz.shape[0]
        pv.c, pv.stride = _shift(xyz, 24, C.c_double), 24
        self._keep = []
        if tags is not None:
            t = np.ascontiguousarray(tags, np.uint16)
            self._keep.append(t)
            pv.tag, pv.tag_stride = _shift(t, 2, C.c_uint16), 2
        if tets is not None or tets_mmg is not None:
            tv = _tets_1based(tets) if tets_mmg is None else np.ascontiguousarray(tets_mmg, np.int32)
            self._keep.append(tv)
            pv.tetra_v, pv.tetra_stride, pv.ne = _ip(tv), 16, tv.shape[0] - 1
        self._chk(self.lib.pmx_upload_points(self.ctx, C.byref(pv)), "pmx_upload_points")
        self.npts = xyz.shape[0]
        # the view's tets are the device's new tets (read by the first run):
        # new_mesh_qual(None) sizes its output by them
        self.n_new_tets = int(pv.ne) if pv.tetra_v else 0

    def upload_point_sources(self, src: np.ndarray | None):
        """Source vertices of the uploaded points (MMG5_Point.src of a ParMmg
        built with USE_POINTMAP): src[j] = the 1-based background vertex the
        j-th point descends from (0 / out of range: unset).  Kept until the
        next upload_points; None forgets them.  Read by run(pointmap=True)."""
        if src is None:
            self._chk(self.lib.pmx_upload_point_sources(self.ctx, None, 4), "pmx_upload_point_sources")
            return
        a = np.ascontiguousarray(src, np.int32)
        if a.shape != (self.npts,):
            raise ValueError("upload_point_sources: one source per uploaded point")
        # the C view is 1-based like the points view (first = 1)
        self._chk(self.lib.pmx_upload_point_sources(self.ctx, _shift(a, 4, C.c_int), 4),
                  "pmx_upload_point_sources")

    def pointmap_stats(self) -> dict:
        """atomicMin operations the last first-incident-element map build
        issued (tet pass, tria pass)."""
        a = (N.i64 * 2)()
        self._chk(self.lib.pmx_pointmap_stats(self.ctx, a), "pmx_pointmap_stats")
        return {"atomics_tets": a[0], "atomics_trias": a[1]}

    def run(self, hsiz: float = 0.0, timing: bool = False, max_walk: int = 0, hint_stride: int = 0,
            flags: int = 0, record_starts: bool = False, pointmap: bool = False):
        """One step (asynchronous; device-side failures surface in
        synchronize()/download()).  flags: ``_native.RUN_*``.  record_starts:
        keep every volume point's walk start tet for starts() (diagnostics;
        the production step does not write it).  pointmap: every walk starts
        from its point's source vertex (upload_point_sources) instead of the
        hint grids."""
        if record_starts:
            flags |= N.RUN_RECORD_STARTS
        if pointmap:
            flags |= N.RUN_POINTMAP
        o = N.RunOpts()
        o.hsiz, o.timing, o.max_walk, o.hint_stride, o.flags = hsiz, int(timing), max_walk, hint_stride, flags
        self._chk(self.lib.pmx_run(self.ctx, C.byref(o)), "pmx_run")

    def download(self, init: list[np.ndarray] | None = None, into: Result | None = None,
                 sols_only: bool = False) -> Result:
        """Results into new arrays (``init`` = values kept where a field is not
        written), or in place into the arrays of ``into`` -- ParMmg's case, whose
        ``met->m`` / ``field->m`` already exist (no allocation per step).
        sols_only: the fields only (what PMMG_interpMetricsAndFields returns;
        elem/status/steps are not copied)."""
        n = self.npts
        if into is not None:
            outs, elem, status, steps = into.sols, into.elem, into.status, into.steps
            if (len(outs) != len(self.sizes) or any(
                    a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != (n, sz)
                    for a, sz in zip(outs, self.sizes)) or any(
                    a.dtype != np.int32 or not a.flags.c_contiguous or a.shape != (n,)
                    for a in (elem, status, steps))):
                raise ValueError("download(into=...): arrays do not match the uploaded step")
        else:
            outs = []
            for i, sz in enumerate(self.sizes):
                outs.append(np.array(init[i], np.float64, copy=True).reshape(n, sz) if init is not None
                            else np.full((n, sz), np.nan))
            elem = np.zeros(n, np.int32)
            status = np.zeros(n, np.int32)
            steps = np.zeros(n, np.int32)
        views = (N.SolView * max(len(self.sizes), 1))()
        for i, (a, sz) in enumerate(zip(outs, self.sizes)):
            views[i].size, views[i].m = sz, _dp(a)
        if sols_only:
            self._chk(self.lib.pmx_download(self.ctx, views, n, None, None, None), "pmx_download")
        else:
            self._chk(self.lib.pmx_download(self.ctx, views, n, _ip(elem), _ip(status), _ip(steps)),
                      "pmx_download")
        return Result(outs, elem, status, steps)

    def interp_more(self, sols: list[np.ndarray], init: list[np.ndarray] | None = None) -> list[np.ndarray]:
        """pmx_interp_more: further solutions of the uploaded background
        ((np+1, size) arrays in Mmg layout, any number of them) onto the points
        the last step located, from that step's elements -- no second walk.
        Returns one (npts, size) array per solution; ``init`` as in
        :meth:`download` (values kept where the reference writes nothing)."""
        arr = [np.ascontiguousarray(s, np.float64) for s in sols]
        if not arr:
            raise ValueError("interp_more: at least one solution")
        arr = [a.reshape(-1, 1) if a.ndim == 1 else a for a in arr]
        for a in arr:
            # (no background yet: the library refuses the call before it reads a row)
            if a.ndim != 2 or (self.bg_np > 0 and a.shape[0] != self.bg_np + 1):
                raise ValueError(f"interp_more: an old field has {a.shape[0]} rows, the uploaded background "
                                 f"has {self.bg_np} vertices (np + 1 = {self.bg_np + 1} rows expected)")
        n = self.npts
        outs = []
        for i, a in enumerate(arr):
            sz = a.shape[1]
            outs.append(np.array(init[i], np.float64, copy=True).reshape(n, sz) if init is not None
                        else np.full((n, sz), np.nan))
        olds = (N.SolView * len(arr))()
        news = (N.SolView * len(arr))()
        for i, (a, o) in enumerate(zip(arr, outs)):
            olds[i].size, olds[i].m = a.shape[1], _dp(a)
            news[i].size, news[i].m = a.shape[1], _dp(o)
        self._chk(self.lib.pmx_interp_more(self.ctx, len(arr), olds, news, n), "pmx_interp_more")
        return outs

    def starts(self) -> np.ndarray:
        s = np.zeros(self.npts, np.int32)
        self._chk(self.lib.pmx_download_starts(self.ctx, _ip(s), len(s)), "pmx_download_starts")
        return s

    def debug_grid(self, which: int = 0) -> tuple[dict, np.ndarray]:
        """The hint grid the last run built (pmx_debug_grid): which 0 the
        volume grid, 1 the tria grid.  Returns ({"dim", "qf" (3,) int, "lo",
        "inv" (3,) float64}, cells (dim[2], dim[1], dim[0]) int32).  Raises
        when the last step built no such grid."""
        d = N.GridDesc()
        n = self.lib.pmx_debug_grid(self.ctx, which, C.byref(d), None, 0)
        self._chk(n, "pmx_debug_grid")
        cells = np.zeros(n, np.int32)
        self._chk(self.lib.pmx_debug_grid(self.ctx, which, C.byref(d), _ip(cells), n), "pmx_debug_grid")
        desc = {"dim": np.array(d.dim, np.int64), "qf": np.array(d.qf, np.int64),
                "lo": np.array(d.lo, np.float64), "inv": np.array(d.inv, np.float64)}
        return desc, cells.reshape(int(d.dim[2]), int(d.dim[1]), int(d.dim[0]))

    def border(self) -> tuple[np.ndarray, np.ndarray]:
        e = np.zeros(self.npts, np.int32)
        v = np.zeros(self.npts, np.int32)
        self._chk(self.lib.pmx_download_border(self.ctx, _ip(e), _ip(v), len(e)), "pmx_download_border")
        return e, v

    def locate_stats(self) -> dict:
        st = N.LocateStats()
        self._chk(self.lib.pmx_locate_stats_get(self.ctx, C.byref(st)), "pmx_locate_stats_get")
        return {f: getattr(st, f) for f, _ in N.LocateStats._fields_}

    def seq_surface_stats(self) -> dict:
        """After a RUN_SEQUENTIAL_SURFACE step: the surface sequence length and
        the queries replayed one by one on the reference's state."""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.lib.pmx_seq_surface_stats(self.ctx, C.byref(a), C.byref(b)), "pmx_seq_surface_stats")
        return {"nseq": a.value, "nreplay": b.value}

    def seq_volume_stats(self) -> dict:
        """After a RUN_SEQUENTIAL_VOLUME step: the volume sequence length and
        the walks replayed one by one on the reference's tet flags."""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.lib.pmx_seq_volume_stats(self.ctx, C.byref(a), C.byref(b)), "pmx_seq_volume_stats")
        return {"nseq": a.value, "nreplay": b.value}

    def wave_stats(self, path: int = 0) -> dict:
        """Lane utilisation of the last step's walks (path 0 volume, 1 surface):
        step_sum / lane_steps, lane_steps = sum over waves of 64 x the wave's
        longest walk; wave_max_hist = waves by their longest walk."""
        st = N.WaveStats()
        self._chk(self.lib.pmx_locate_wave_stats(self.ctx, path, C.byref(st)), "pmx_locate_wave_stats")
        d = {f: getattr(st, f) for f, _ in N.WaveStats._fields_}
        d["wave_max_hist"] = list(st.wave_max_hist)
        d["lane_utilization"] = st.step_sum / st.lane_steps if st.lane_steps else None
        d["mean_wave_max"] = st.lane_steps / 64 / st.waves if st.waves else None
        return d

    def kernel_ms(self, which: int) -> float:
        return self.lib.pmx_kernel_ms(self.ctx, which)

    def timing_reset(self):
        self.lib.pmx_timing_reset(self.ctx)

    def device_buffer(self, which: int) -> int:
        return self.lib.pmx_device_buffer(self.ctx, which) or 0

    # ---- background topology (MMG3D_hashTetra, MMG5_chkBdryTria + hashTria) --
    def build_adja(self, tet: np.ndarray, np_: int) -> np.ndarray:
        """Tet face adjacency on the device, Mmg layout (4*ne+5 ints)."""
        t = np.ascontiguousarray(tet, np.int32)
        ne = t.shape[0] - 1
        adja = np.zeros(4 * ne + 5, np.int32)
        self._chk(self.lib.pmx_build_adja(self.ctx, ne, np_, t.ctypes.data, 16, adja.ctypes.data),
                  "pmx_build_adja")
        return adja

    def build_bdry(self, tet: np.ndarray, np_: int, adja: np.ndarray):
        """Boundary trias ((nt+1, 3), row 0 unused) and their adjacency."""
        t = np.ascontiguousarray(tet, np.int32)
        a = np.ascontiguousarray(adja, np.int32)
        ne = t.shape[0] - 1
        maxnt = 4 * ne
        tria = np.zeros((maxnt + 1, 3), np.int32)
        adjt = np.zeros(3 * maxnt + 4, np.int32)
        nt = self.lib.pmx_build_bdry(self.ctx, ne, np_, t.ctypes.data, 16, a.ctypes.data,
                                     tria.ctypes.data, maxnt, adjt.ctypes.data)
        if nt < 0:
            raise RuntimeError(f"pmx_build_bdry: {self.lib.pmx_last_error(self.ctx).decode()}")
        return np.ascontiguousarray(tria[: nt + 1]), np.ascontiguousarray(adjt[: 3 * nt + 4])

    def topo_ms(self) -> float:
        return self.lib.pmx_topo_ms(self.ctx)

    # ---- reference-shaped entry points --------------------------------------
    def interp_metrics_and_fields(self, groups: list[dict], input_met: int = 1,
                                  perm_nod_glob: np.ndarray | None = None) -> int:
        """PMMG_interpMetricsAndFields over ``groups``; each group is a dict with
        keys ``old_mesh`` (Mesh), ``old_met`` ((np+1,size) or None),
        ``old_fields`` (list), ``xyz`` (new points, (np+1,3) Mmg layout),
        ``tags`` (uint16, np+1), ``met`` / ``fields`` (output arrays in Mmg
        layout, written in place), ``hsiz``, optionally ``tets`` (the new
        tets, (ne+1, 4) in Mmg's 1-based layout: the orphan rule and, with
        PMX_SEQUENTIAL set, the reference's visit order) and ``src`` (int32,
        np+1: each new point's source vertex in the old mesh, MMG5_Point.src
        of a USE_POINTMAP build -- that group's walks start from it)."""
        keep = []
        G = (N.Group * len(groups))()
        srcs = (N.PointSources * max(len(groups), 1))()
        any_src = False
        for (g, d), ps in zip(zip(G, groups), srcs):
            if d.get("src") is not None:
                sa = np.ascontiguousarray(d["src"], np.int32)
                keep.append(sa)
                ps.src, ps.stride = _ip(sa), 4
                any_src = True
            xyz = np.ascontiguousarray(d["xyz"], np.float64)
            tags = np.ascontiguousarray(d["tags"], np.uint16)
            keep += [xyz, tags]
            g.points.first, g.points.last = 1, xyz.shape[0] - 1
            g.points.c, g.points.stride = _dp(xyz), 24
            g.points.tag, g.points.tag_stride = tags.ctypes.data_as(N.u16ptr), 2
            if d.get("tets") is not None:             # Mmg layout: (ne+1, 4), 1-based, v[0] = 0 deleted
                tv = np.ascontiguousarray(d["tets"], np.int32)
                keep.append(tv)
                g.points.tetra_v, g.points.tetra_stride, g.points.ne = _ip(tv), 16, tv.shape[0] - 1
            g.hsiz = d.get("hsiz", 0.0)
            om = mesh_view(d["old_mesh"])
            keep.append(om)
            g.old_mesh = om

            def sv(a):
                v = N.SolView()
                v.size, v.m = a.shape[1], _dp(a)
                return v
            if d.get("met") is not None and d.get("old_met") is not None:
                g.met = C.pointer(sv(d["met"]))
                g.old_met = C.pointer(sv(d["old_met"]))
                keep += [g.met, g.old_met]
            fl = d.get("fields") or []
            ofl = d.get("old_fields") or []
            g.nsols = len(fl)
            if fl:
                fa = (N.SolView * len(fl))(*[sv(a) for a in fl])
                ofa = (N.SolView * len(ofl))(*[sv(a) for a in ofl])
                keep += [fa, ofa]
                g.fields = C.cast(fa, C.POINTER(N.SolView))
                g.old_fields = C.cast(ofa, C.POINTER(N.SolView))
        perm = None
        if perm_nod_glob is not None:
            perm = np.ascontiguousarray(perm_nod_glob, np.int32)
        self.bg_np = 0                       # the contexts' backgrounds become the groups'
        if any_src:
            # the seam with sources takes one context per group: alternate
            # between this one and a second one, as the plain call does
            if len(groups) > 1 and self._peer is None:
                self._peer = Transfer(self.device)
            ctxs = (C.c_void_p * len(groups))(*[self._peer.ctx if (len(groups) > 1 and i & 1) else self.ctx
                                                for i in range(len(groups))])
            return self.lib.PMX_interpMetricsAndFields_groups_src(ctxs, len(groups), G, srcs, _ip(perm),
                                                                  input_met)
        return self.lib.PMX_interpMetricsAndFields(self.ctx, len(groups), G, _ip(perm), input_met)

    # ---- statistics -----------------------------------------------------------
    def upload_point_tags(self, tags: np.ndarray | None):
        """MMG5_Point.tag of the uploaded background, (np+1,) (ridge points for
        the length filter and OUTQUA's nrid)."""
        t = None if tags is None else np.ascontiguousarray(tags, np.uint16)
        self._keep_tags = t
        self._chk(self.lib.pmx_upload_point_tags(self.ctx, t.ctypes.data_as(N.u16ptr) if t is not None
                                                 else None, 2), "pmx_upload_point_tags")

    def tetra_qual(self, ne: int, met_rid_typ: int = 0) -> np.ndarray:
        """MMG3D_tetraQual(mesh, met, metRidTyp) of the uploaded group."""
        q = np.zeros(ne + 1)
        self._chk(self.lib.pmx_tetra_qual(self.ctx, met_rid_typ, _dp(q), len(q)), "pmx_tetra_qual")
        return q

    def count_nodes(self, idx_ip=None, idx_comm=None, intvalues=None, base: int = 1) -> int:
        """PMMG_count_nodes_par on the uploaded group; intvalues is updated in place."""
        n_grp = 0 if idx_ip is None else len(idx_ip)
        ip = np.ascontiguousarray(idx_ip if idx_ip is not None else [], np.int32)
        ic = np.ascontiguousarray(idx_comm if idx_comm is not None else [], np.int32)
        iv = intvalues if intvalues is not None else np.zeros(0, np.int32)
        assert iv.dtype == np.int32 and iv.flags.c_contiguous
        out = C.c_int64()
        self._chk(self.lib.pmx_count_nodes(self.ctx, _ip(ip), _ip(ic), n_grp, _ip(iv), len(iv), base,
                                           C.byref(out)), "pmx_count_nodes")
        return out.value

    @staticmethod
    def _qdict(st) -> dict:
        d = {f: getattr(st, f) for f, _ in N.QualStats._fields_}
        d["his"] = list(st.his)
        return d

    @staticmethod
    def _ldict(st) -> dict:
        d = {f: getattr(st, f) for f, _ in N.LenStats._fields_}
        d["hl"] = list(st.hl)
        return d

    def qualhisto(self, opt: int = N.INQUA) -> dict:
        st = N.QualStats()
        self._chk(self.lib.pmx_qualhisto(self.ctx, opt, C.byref(st)), "pmx_qualhisto")
        return self._qdict(st)

    def qualhisto_device(self, dev_ptr: int, opt: int = N.INQUA, use_stored: bool = False):
        self._chk(self.lib.pmx_qualhisto_device(self.ctx, opt, int(use_stored), C.c_void_p(dev_ptr)),
                  "pmx_qualhisto_device")

    @staticmethod
    def _par(par: dict | None):
        if par is None:
            return None, []
        a = np.ascontiguousarray(par["a"], np.int32)
        b = np.ascontiguousarray(par["b"], np.int32)
        o = np.ascontiguousarray(par["owner"], np.int32)
        pe = N.ParEdges()
        pe.n, pe.a, pe.b, pe.owner = len(a), _ip(a), _ip(b), _ip(o)
        pe.myrank, pe.exact_once = int(par.get("myrank", 0)), int(par.get("exact_once", 0))
        keep = [a, b, o, pe]
        if par.get("tag") is not None:
            t = np.ascontiguousarray(par["tag"], np.uint16)
            pe.tag = t.ctypes.data_as(N.u16ptr)
            keep.append(t)
        return C.byref(pe), keep

    def upload_surface(self, surface: dict | None):
        """Mmg's surface data of the uploaded group (pmx_upload_surface):
        {"xt" (ne+1,) tetra[k].xt, "xtag" (nxt+1, 6) xtetra[x].tag, "n" (np+1, 3)
        point[i].n, "xp" (np+1,) point[i].xp, "n1"/"n2" (nxp+1, 3) xpoint[x].n1/n2};
        None: no surface data (no xTetra, zero normals)."""
        if surface is None:
            self._chk(self.lib.pmx_upload_surface(self.ctx, None), "pmx_upload_surface")
            return
        xt = np.ascontiguousarray(surface["xt"], np.int32)
        xtag = np.ascontiguousarray(surface["xtag"], np.uint16).reshape(-1, 6)
        n = np.ascontiguousarray(surface["n"], np.float64).reshape(-1, 3)
        xp = np.ascontiguousarray(surface["xp"], np.int32)
        n1 = np.ascontiguousarray(surface["n1"], np.float64).reshape(-1, 3)
        n2 = np.ascontiguousarray(surface["n2"], np.float64).reshape(-1, 3)
        sv = N.SurfaceView()
        sv.nxt, sv.nxp = xtag.shape[0] - 1, n1.shape[0] - 1
        sv.tetra_xt, sv.tetra_stride = _ip(xt), 4
        sv.xtetra_tag, sv.xtetra_stride = xtag.ctypes.data_as(N.u16ptr), 12
        sv.point_n, sv.point_xp, sv.point_stride = _dp(n), _ip(xp), 24
        # point_n / point_xp share one stride in the ABI (MMG5_Point): pack them
        rec = np.zeros(n.shape[0], dtype=[("n", np.float64, 3), ("xp", np.int32), ("pad", np.int32)])
        rec["n"], rec["xp"] = n, xp
        sv.point_n = C.cast(C.c_void_p(rec.ctypes.data), N.dptr)
        sv.point_xp = C.cast(C.c_void_p(rec.ctypes.data + 24), N.iptr)
        sv.point_stride = rec.dtype.itemsize
        sv.xpoint_n1, sv.xpoint_n2, sv.xpoint_stride = _dp(n1), _dp(n2), 24
        self._chk(self.lib.pmx_upload_surface(self.ctx, C.byref(sv)), "pmx_upload_surface")

    def prilen(self, met_rid_typ: int = 0, par: dict | None = None) -> dict:
        """par: {"a", "b", "owner", "myrank", "exact_once"} (distributed PMMG_prilen)."""
        st = N.LenStats()
        pp, keep = self._par(par)
        self._chk(self.lib.pmx_prilen(self.ctx, met_rid_typ, pp, C.byref(st)), "pmx_prilen")
        del keep
        return self._ldict(st)

    def prilen_device(self, dev_ptr: int, met_rid_typ: int = 0, par: dict | None = None):
        pp, keep = self._par(par)
        self._chk(self.lib.pmx_prilen_device(self.ctx, met_rid_typ, pp, C.c_void_p(dev_ptr)),
                  "pmx_prilen_device")
        del keep

    def metis_graph(self, met_rid_typ: int = 0, weights: bool = True):
        """PMMG_graph_meshElts2metis of the uploaded (or promoted) group
        (pmx_metis_graph): (xadj (ne+1,), adjncy (nadjncy,), adjwgt (nadjncy,)
        or None) as int32, the idx_t of a default Metis build.  weights=False:
        the reference's *adjwgt == NULL (distribution time, last iteration)."""
        ne = self.bg_ne
        xadj = np.empty(ne + 1, np.int32)
        adjncy = np.empty(max(4 * ne, 1), np.int32)
        adjwgt = np.empty(max(4 * ne, 1), np.int32) if weights else None
        n = C.c_int64(0)
        i32 = lambda a: a.ctypes.data_as(N.i32ptr) if a is not None else None
        self._chk(self.lib.pmx_metis_graph(self.ctx, met_rid_typ, i32(xadj), i32(adjncy), i32(adjwgt),
                                           len(adjncy), C.byref(n)), "pmx_metis_graph")
        return xadj, adjncy[: n.value], (adjwgt[: n.value] if weights else None)

    def face_weights(self, faces: np.ndarray, met_rid_typ: int = 0) -> np.ndarray:
        """PMMG_computeWgt as doubles for the listed faces of the uploaded
        group, faces[i] = 12*ie + 3*ifac (+ iloc): pmx_face_weights."""
        f = np.ascontiguousarray(faces, np.int32)
        w = np.zeros(len(f))
        self._chk(self.lib.pmx_face_weights(self.ctx, met_rid_typ, len(f), _ip(f), _dp(w)), "pmx_face_weights")
        return w

    def contiguity(self, part: np.ndarray | None = None, nparts: int = 1):
        """The face-connected components of the uploaded (or promoted) group
        restricted to equal part values (pmx_contiguity): (ncomp, counts
        (nparts,), label (ne,)) with label[k-1] the smallest 1-based tet of tet
        k's component.  part=None: one colour, PMMG_check_grps_contiguity."""
        ne = self.bg_ne
        p = None if part is None else np.ascontiguousarray(part, np.int32)
        if p is not None and p.shape != (ne,):
            raise ValueError(f"part has shape {p.shape}, the group has {ne} tets")
        counts = np.zeros(max(nparts, 0), np.int32)
        label = np.zeros(ne, np.int32)
        n = C.c_int64(0)
        i32 = lambda a: a.ctypes.data_as(N.i32ptr) if a is not None and a.size else None
        self._chk(self.lib.pmx_contiguity(self.ctx, i32(p), nparts, i32(counts), i32(label), C.byref(n)),
                  "pmx_contiguity")
        return n.value, counts, label

    def fix_contiguity(self, part: np.ndarray, colors_or_n, replay_steps: int = 0):
        """PMMG_fix_contiguity_split / _centralized / PMMG_fix_contiguity on a
        copy of part (pmx_fix_contiguity): (part, stats).  colors_or_n: the
        number of colours (0..n-1, in that order) or the list of colours to
        process in order; stats: the fields of pmx_contig_stats as a dict."""
        ne = self.bg_ne
        p = np.array(part, np.int32, order="C")
        if p.shape != (ne,):
            raise ValueError(f"part has shape {p.shape}, the group has {ne} tets")
        if np.ndim(colors_or_n) == 0:
            ncol, col = int(colors_or_n), None
        else:
            col = np.ascontiguousarray(colors_or_n, np.int32)
            ncol = len(col)
        st = N.ContigStats()
        self._chk(self.lib.pmx_fix_contiguity(self.ctx, p.ctypes.data_as(N.i32ptr), ncol,
                                              col.ctypes.data_as(N.i32ptr) if col is not None else None,
                                              replay_steps, C.byref(st)), "pmx_fix_contiguity")
        return p, {f: getattr(st, f) for f, _ in st._fields_}

    @staticmethod
    def _split_comm(comm: dict | None):
        """comm as a pmx_split_comm, with the arrays it points into."""
        comm = comm or {}
        arr = {k: np.ascontiguousarray(comm.get(k, np.zeros(0)), np.int32)
               for k in ("face_index1", "face_index2", "node_index1", "node_index2")}
        if len(arr["face_index1"]) != len(arr["face_index2"]) or len(arr["node_index1"]) != len(arr["node_index2"]):
            raise ValueError("index1 and index2 of a communicator differ in length")
        c = N.SplitComm()
        c.nface, c.nnode = len(arr["face_index1"]), len(arr["node_index1"])
        for k, a in arr.items():
            setattr(c, k, _ip(a) if a.size else None)
        c.int_face_nitem = int(comm.get("int_face_nitem", 0))
        c.int_node_nitem = int(comm.get("int_node_nitem", 0))
        return c, arr

    def split_groups(self, part: np.ndarray, ngrp: int, comm: dict | None = None) -> dict:
        """PMMG_split_eachGrp of the uploaded (or promoted) group by part
        (pmx_split_groups): the plan stays on the device, split_fetch returns
        one group.  comm: the old group's internal communicators, any of
        face_index1/2, node_index1/2, int_face_nitem, int_node_nitem.  Returns
        sizes ((ngrp, 4) int64: ne, np, nface, nnode per group), tet_new (ne,)
        and the two final nitem."""
        ne = self.bg_ne
        p = np.ascontiguousarray(part, np.int32)
        if p.shape != (ne,):
            raise ValueError(f"part has shape {p.shape}, the group has {ne} tets")
        c, _keep = self._split_comm(comm)
        sizes = (N.SplitSizes * max(ngrp, 1))()
        tet_new = np.zeros(ne, np.int32)
        fn, nn = C.c_int64(0), C.c_int64(0)
        self._split_sizes = None
        self._chk(self.lib.pmx_split_groups(self.ctx, p.ctypes.data_as(N.i32ptr), ngrp, C.byref(c), sizes,
                                            _ip(tet_new) if ne else None, C.byref(fn), C.byref(nn)),
                  "pmx_split_groups")
        sz = np.array([[s.ne, s.np, s.nface, s.nnode] for s in sizes[:ngrp]], np.int64).reshape(ngrp, 4)
        self._split_sizes = sz
        return {"sizes": sz, "tet_new": tet_new, "int_face_nitem": fn.value, "int_node_nitem": nn.value}

    def split_fetch(self, g: int, data: bool = True) -> dict:
        """One new group of the last split_groups (pmx_split_fetch): tet_old
        (ne,), tetra_v ((ne+1, 4), row 0 unused), adja (4*ne+5, Mmg layout),
        point_old (np,), face_index1/2, node_index1/2; with data also xyz
        ((np+1, 3), row 0 unused, as Mesh wants it) and sols, the rows of every
        uploaded solution ((np+1, size) each)."""
        sz = getattr(self, "_split_sizes", None)
        if sz is None or not 0 <= g < len(sz):
            neg = npg = nf = nn = 0       # the library refuses: no plan, or g out of range
        else:
            neg, npg, nf, nn = (int(v) for v in sz[g])
        # the library writes every entry but row 0 of the 1-based arrays
        d = {"tet_old": np.empty(neg, np.int32), "tetra_v": np.empty((neg + 1, 4), np.int32),
             "adja": np.empty(4 * neg + 5, np.int32), "point_old": np.empty(npg, np.int32),
             "face_index1": np.empty(nf, np.int32), "face_index2": np.empty(nf, np.int32),
             "node_index1": np.empty(nn, np.int32), "node_index2": np.empty(nn, np.int32)}
        d["tetra_v"][0] = 0
        o = N.SplitOut()
        for k, a in d.items():
            setattr(o, k, _ip(a))
        if data:
            d["xyz"] = np.empty((npg + 1, 3))
            d["sols"] = [np.empty((npg + 1, s)) for s in self.sizes]
            for a in [d["xyz"]] + d["sols"]:
                a[0] = 0.0
            o.xyz = _dp(d["xyz"])
            views = (N.SolView * max(len(self.sizes), 1))()
            for i, a in enumerate(d["sols"]):
                views[i].size = self.sizes[i]
                views[i].m = _dp(a)
            o.nsol = len(self.sizes)
            o.sols = views
        self._chk(self.lib.pmx_split_fetch(self.ctx, g, C.byref(o)), "pmx_split_fetch")
        return d

    def split_release(self):
        """Free the plan's device memory (pmx_split_release)."""
        self._split_sizes = None
        self._chk(self.lib.pmx_split_release(self.ctx), "pmx_split_release")

    def split_adopt(self, g: int, dst: "Transfer", imet: int = 0, surface: bool = True, hausd: float = 0.01):
        """Group g of the last split_groups becomes dst's uploaded group on the
        device (pmx_split_adopt), as dst.upload_background(group mesh,
        adja=False) of split_fetch(g) would leave it -- with surface the
        boundary trias and their adjacency are built on the device, without it
        nt = 0.  This context's plan and background are untouched.  imet:
        index of the metric among the solutions, or -1."""
        sz = getattr(self, "_split_sizes", None)
        if sz is None:                   # before dst changes: its sizes below come from split_groups' table
            raise RuntimeError("pmx_split_adopt: no plan: call split_groups")
        r = self.lib.pmx_split_adopt(self.ctx, g, dst.ctx, imet if self.sizes else -1, int(surface), hausd)
        if not r:
            raise RuntimeError(f"pmx_split_adopt: {self.lib.pmx_last_error(dst.ctx).decode()}")
        dst._split_sizes = None
        dst.sizes = list(self.sizes)
        dst.bg_ne, dst.bg_np = int(sz[g][0]), int(sz[g][1])
        dst.bg_nt = int(self.lib.pmx_download_surface(dst.ctx, None, 0, None))   # built on the device

    def download_surface(self):
        """The installed background's boundary trias as the device holds them
        (pmx_download_surface): (tria (nt+1, 3), row 0 unused, adjt (3*nt+4,)),
        the numbering of a surface point's downloaded elem."""
        nt = self.lib.pmx_download_surface(self.ctx, None, 0, None)      # the size query
        tria = np.zeros((max(nt, 0) + 1, 3), np.int32)
        adjt = np.zeros(3 * max(nt, 0) + 4, np.int32)
        if nt < 0 or self.lib.pmx_download_surface(self.ctx, _ip(tria), nt, _ip(adjt)) != nt:
            raise RuntimeError(f"pmx_download_surface: {self.lib.pmx_last_error(self.ctx).decode()}")
        self.bg_nt = int(nt)
        return tria, adjt

    # ---- group merge ----------------------------------------------------------
    def _merge_views(self, groups: list[dict], comm: dict | None = None):
        """The pmx_merge_group array, nsol, the pmx_merge_comm and the numpy
        arrays they point into (kept alive by the caller), from the dicts
        merge_groups takes."""
        comm = comm or {}
        ngrp = len(groups)
        keep = []
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        gv = (N.MergeGroup * max(ngrp, 1))()
        held = lambda d: d.get("held")
        nsol = (len(held(groups[0]).sizes) if held(groups[0]) is not None else len(groups[0]["sols"])) if ngrp else 0
        sol_sizes = []
        sizes = []
        for g, d in enumerate(groups):
            idx = {k: i32(d.get(k, np.zeros(0))) for k in ("node_index1", "node_index2", "face_index1", "face_index2")}
            if len(idx["node_index1"]) != len(idx["node_index2"]) or len(idx["face_index1"]) != len(idx["face_index2"]):
                raise ValueError("index1 and index2 of a communicator differ in length")
            v = gv[g]
            v.nnode, v.nface = len(idx["node_index1"]), len(idx["face_index1"])
            if held(d) is not None:
                # the context's group: only the index arrays are read, in its own numbering
                keep += [idx]
                sizes.append((held(d).bg_np, held(d).bg_ne))
                sol_sizes = sol_sizes if g else [int(s) for s in held(d).sizes]
            else:
                tv, xyz = i32(d["tetra_v"]), np.ascontiguousarray(d["xyz"], np.float64)
                sols = [np.ascontiguousarray(s, np.float64) for s in d["sols"]]
                if len(sols) != nsol:
                    raise ValueError("the groups differ in their number of solutions")
                views = (N.SolView * max(nsol, 1))()
                for i, a in enumerate(sols):
                    views[i].size = a.shape[1] if a.ndim == 2 else 1
                    views[i].m = _dp(a)
                keep += [tv, xyz, sols, views, idx]
                v.np, v.ne = xyz.shape[0] - 1, tv.shape[0] - 1
                v.point_c, v.point_stride = _dp(xyz), 24
                v.tetra_v, v.tetra_stride = _ip(tv), 16
                v.sols = views
                sizes.append((int(v.np), int(v.ne)))
                sol_sizes = sol_sizes if g else [int(w.size) for w in views[:nsol]]
            for k, a in idx.items():
                setattr(v, k, _ip(a) if a.size else None)
        c = N.MergeComm()
        c.int_node_nitem = int(comm.get("int_node_nitem", 0))
        c.int_face_nitem = int(comm.get("int_face_nitem", 0))
        ext = {}
        for kind in ("node", "face"):
            lists = [i32(a) for a in comm.get("ext_" + kind, [])]
            off = np.zeros(len(lists) + 1, np.int64)
            off[1:] = np.cumsum([len(a) for a in lists])
            items = np.concatenate(lists) if lists else np.zeros(0, np.int32)
            ext[kind] = (off, i32(items))
            setattr(c, "next_" + kind, len(lists))
            setattr(c, kind + "_off", off.ctypes.data_as(C.POINTER(N.i64)) if lists else None)
            setattr(c, kind + "_items", _ip(ext[kind][1]) if items.size else None)
        meta = {"sol_sizes": sol_sizes, "nen": len(ext["node"][1]), "nef": len(ext["face"][1]),
                "np": [n for n, _ in sizes], "ne": [n for _, n in sizes]}
        return gv, nsol, c, meta, keep + [ext]

    def merge_groups(self, groups: list[dict], comm: dict | None = None) -> dict:
        """PMMG_merge_grps of a rank's groups (pmx_merge_groups): the merged
        group stays on the device; merge_fetch returns it, merge_adopt makes it
        the uploaded group.  groups: the dicts split_fetch returns (tetra_v,
        xyz, sols, node_index1/2, face_index1/2).  comm: int_node_nitem,
        int_face_nitem and the external communicators ext_node / ext_face,
        lists of int_comm_index arrays.  Returns sizes ((4,) int64: np, ne,
        nnode, nface of the merged group)."""
        gv, nsol, c, meta, keep = self._merge_views(groups, comm)
        sz = N.MergeSizes()
        self._merge = None
        self._chk(self.lib.pmx_merge_groups(self.ctx, len(groups), gv, nsol, C.byref(c), C.byref(sz)),
                  "pmx_merge_groups")
        sizes = np.array([sz.np, sz.ne, sz.nnode, sz.nface], np.int64)
        self._merge = dict(meta, sizes=sizes)
        return {"sizes": sizes}

    def merge_groups_from(self, sources: list[dict], comm: dict | None = None) -> dict:
        """merge_groups with sources that contexts hold (pmx_merge_groups_from).
        A source is a dict as merge_groups takes it, or {"held": a Transfer on
        this device, node_index1/2, face_index1/2}: the group that context
        holds as its background, read on the device; its index arrays are in
        that group's own numbering.  A held group may have unused points and
        deleted tets: they are dropped, merge_maps(g) -- sized by the held
        group's own np and ne -- holds 0 for them, and tet_old / point_old of
        merge_fetch are ids in the held group's own numbering.  Returns sizes
        as merge_groups does."""
        gv, nsol, c, meta, keep = self._merge_views(sources, comm)
        sv = (N.MergeSource * max(len(sources), 1))()
        for g, d in enumerate(sources):
            sv[g].held = d["held"].ctx if d.get("held") is not None else None
            sv[g].g = gv[g]
        sz = N.MergeSizes()
        self._merge = None
        self._chk(self.lib.pmx_merge_groups_from(self.ctx, len(sources), sv, nsol, C.byref(c), C.byref(sz)),
                  "pmx_merge_groups_from")
        sizes = np.array([sz.np, sz.ne, sz.nnode, sz.nface], np.int64)
        self._merge = dict(meta, sizes=sizes)
        return {"sizes": sizes}

    def merge_fetch(self, data: bool = True) -> dict:
        """The merged group of the last merge_groups (pmx_merge_fetch): tetra_v
        ((ne+1, 4), row 0 unused), tet_group, tet_old (ne,), point_group,
        point_old (np,), node_index1/2, face_index1/2, ext_node_items,
        ext_face_items (the external communicators' items, concatenated); with
        data also xyz ((np+1, 3)) and sols ((np+1, size) each)."""
        mg = getattr(self, "_merge", None)
        npm, nem, nn, nf = (int(v) for v in mg["sizes"]) if mg else (0, 0, 0, 0)
        nen, nef = (mg["nen"], mg["nef"]) if mg else (0, 0)
        d = {"tetra_v": np.empty((nem + 1, 4), np.int32), "tet_group": np.empty(nem, np.int32),
             "tet_old": np.empty(nem, np.int32), "point_group": np.empty(npm, np.int32),
             "point_old": np.empty(npm, np.int32), "node_index1": np.empty(nn, np.int32),
             "node_index2": np.empty(nn, np.int32), "face_index1": np.empty(nf, np.int32),
             "face_index2": np.empty(nf, np.int32), "ext_node_items": np.empty(nen, np.int32),
             "ext_face_items": np.empty(nef, np.int32)}
        d["tetra_v"][0] = 0
        o = N.MergeOut()
        for k, a in d.items():
            setattr(o, k, _ip(a))
        if data:
            sizes = mg["sol_sizes"] if mg else []
            d["xyz"] = np.empty((npm + 1, 3))
            d["sols"] = [np.empty((npm + 1, s)) for s in sizes]
            for a in [d["xyz"]] + d["sols"]:
                a[0] = 0.0
            o.xyz = _dp(d["xyz"])
            views = (N.SolView * max(len(sizes), 1))()
            for i, a in enumerate(d["sols"]):
                views[i].size = sizes[i]
                views[i].m = _dp(a)
            o.nsol = len(sizes)
            o.sols = views
        self._chk(self.lib.pmx_merge_fetch(self.ctx, C.byref(o)), "pmx_merge_fetch")
        return d

    def merge_maps(self, g: int):
        """Group g's local-to-merged maps (pmx_merge_maps): point_new (np_g,)
        and tet_new (ne_g,), local entity k at k-1."""
        mg = getattr(self, "_merge", None)
        ok = mg is not None and 0 <= g < len(mg["np"])
        pn = np.empty(mg["np"][g] if ok else 0, np.int32)
        tn = np.empty(mg["ne"][g] if ok else 0, np.int32)
        self._chk(self.lib.pmx_merge_maps(self.ctx, g, _ip(pn), _ip(tn)), "pmx_merge_maps")
        return pn, tn

    def merge_adopt(self, imet: int = 0):
        """The merged group becomes the uploaded group on the device
        (pmx_merge_adopt), as upload_background(merged mesh, adja=False) would
        leave it; imet: index of the metric among the solutions, or -1."""
        mg = getattr(self, "_merge", None)
        self._chk(self.lib.pmx_merge_adopt(self.ctx, imet if mg and mg["sol_sizes"] else -1), "pmx_merge_adopt")
        self._split_sizes = None
        self.sizes = list(mg["sol_sizes"])
        self.bg_np, self.bg_ne = int(mg["sizes"][0]), int(mg["sizes"][1])
        self.bg_nt = 0

    def merge_release(self):
        """Free the merge plan's device memory (pmx_merge_release)."""
        self._merge = None
        self._chk(self.lib.pmx_merge_release(self.ctx), "pmx_merge_release")

    # ---- interface displacement ------------------------------------------------
    def moveifc_begin(self, tet_group: np.ndarray | None, map: dict) -> int:
        """PMMG_set_color_tetra + PMMG_mark_interfacePoints on the uploaded (or
        adopted) group (pmx_moveifc_begin): the front points.  tet_group: (ne,)
        old group per tet, None = the live merge plan's, read on the device.
        map: nprocs, myrank, displsgrp (nprocs + 1,), mapgrp."""
        ne = self.bg_ne
        tg = None if tet_group is None else np.ascontiguousarray(tet_group, np.int32)
        if tg is not None and tg.shape != (ne,):
            raise ValueError(f"tet_group has shape {tg.shape}, the group has {ne} tets")
        nprocs, myrank = int(map.get("nprocs", 1)), int(map.get("myrank", 0))
        displs = np.ascontiguousarray(map["displsgrp"], np.int32)
        mapgrp = np.ascontiguousarray(map["mapgrp"], np.int32)
        if displs.shape != (nprocs + 1,) or not 0 <= myrank < nprocs:
            raise ValueError("displsgrp wants nprocs + 1 entries, myrank lies in 0..nprocs-1")
        if len(mapgrp) != int(displs[-1]):
            raise ValueError("mapgrp wants displsgrp[nprocs] entries")
        mp = N.MoveIfcMap(nprocs, myrank, int(map.get("nold_grp", displs[myrank + 1] - displs[myrank])),
                          _ip(displs), _ip(mapgrp) if mapgrp.size else None)
        nf = C.c_int64(0)
        self._moveifc = None
        self._chk(self.lib.pmx_moveifc_begin(self.ctx, tg.ctypes.data_as(N.i32ptr) if tg is not None else None,
                                             C.byref(mp), C.byref(nf)), "pmx_moveifc_begin")
        self._moveifc = {"nold_grp": mp.nold_grp, "nprocs": nprocs, "myrank": myrank, "ne": ne, "np": self.bg_np,
                         "ngrps_all": int(displs[-1])}
        return nf.value

    def _moveifc_state(self) -> dict:
        return getattr(self, "_moveifc", None) or {"nold_grp": 0, "nprocs": 1, "myrank": 0, "ne": self.bg_ne,
                                                   "np": self.bg_np}

    def moveifc_colors(self, ip: np.ndarray) -> np.ndarray:
        """The colours (tmp) of the listed 1-based points (pmx_moveifc_get_colors)."""
        p = np.ascontiguousarray(ip, np.int32)
        col = np.zeros(len(p), np.int32)
        self._chk(self.lib.pmx_moveifc_get_colors(self.ctx, len(p), _ip(p) if p.size else None,
                                                  _ip(col) if p.size else None), "pmx_moveifc_get_colors")
        return col

    def moveifc_set_colors(self, ip: np.ndarray, color: np.ndarray):
        """The listed points take the colours and join the front
        (pmx_moveifc_set_colors)."""
        p = np.ascontiguousarray(ip, np.int32)
        col = np.ascontiguousarray(color, np.int32)
        if p.shape != col.shape:
            raise ValueError("ip and color differ in length")
        self._chk(self.lib.pmx_moveifc_set_colors(self.ctx, len(p), _ip(p) if p.size else None,
                                                  _ip(col) if p.size else None), "pmx_moveifc_set_colors")

    def moveifc_layer(self, seq_steps: int = 0) -> dict:
        """One layer of PMMG_part_moveInterfaces (pmx_moveifc_layer): its stats
        as a dict.  A ball overflow raises; the state is the layer's start."""
        st = N.MoveIfcStats()
        self._moveifc_last = st
        self._chk(self.lib.pmx_moveifc_layer(self.ctx, seq_steps, C.byref(st)), "pmx_moveifc_layer")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def moveifc_marks(self) -> np.ndarray:
        """The tet marks (ne,), the input of fix_contiguity (pmx_moveifc_marks)."""
        mk = np.zeros(self._moveifc_state()["ne"], np.int32)
        self._chk(self.lib.pmx_moveifc_marks(self.ctx, mk.ctypes.data_as(N.i32ptr) if mk.size else
                                             (C.c_int32 * 1)()), "pmx_moveifc_marks")
        return mk

    def moveifc_points(self):
        """(tmp, s, front), (np,) each: the colour, the slot 4*tet + iloc and
        the front flag of every point (pmx_moveifc_points)."""
        n = self._moveifc_state()["np"]
        tmp, s, fr = (np.zeros(n, np.int32) for _ in range(3))
        self._chk(self.lib.pmx_moveifc_points(self.ctx, _ip(tmp) if n else None, _ip(s) if n else None,
                                              _ip(fr) if n else None), "pmx_moveifc_points")
        return tmp, s, fr

    def moveifc_groups(self):
        """(negrp, nemin) of the local groups (pmx_moveifc_groups)."""
        n = self._moveifc_state()["nold_grp"]
        a, b = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self._chk(self.lib.pmx_moveifc_groups(self.ctx, _ip(a), _ip(b)), "pmx_moveifc_groups")
        return a[:n], b[:n]

    def moveifc_part(self, mark: np.ndarray | None = None, target: int = N.GRPSPL_MMG_TARGET, ngrps_all=None):
        """PMMG_part_getInterfaces (pmx_moveifc_part): (part (ne,), ngrp).
        mark: the marks after fix_contiguity, None = the device's."""
        ne = self._moveifc_state()["ne"]
        mk = None if mark is None else np.ascontiguousarray(mark, np.int32)
        if mk is not None and mk.shape != (ne,):
            raise ValueError(f"mark has shape {mk.shape}, the group has {ne} tets")
        ng = None if ngrps_all is None else np.ascontiguousarray(ngrps_all, np.int32)
        if ng is not None and len(ng) != self._moveifc_state()["nprocs"]:
            raise ValueError("ngrps_all wants nprocs entries")
        part = np.zeros(max(ne, 1), np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.pmx_moveifc_part(self.ctx, mk.ctypes.data_as(N.i32ptr) if mk is not None and ne else None,
                                            target, _ip(ng) if ng is not None else None,
                                            part.ctypes.data_as(N.i32ptr), C.byref(n)), "pmx_moveifc_part")
        return part[:ne], n.value

    @staticmethod
    def _stats(st) -> dict:
        return {f: getattr(st, f) for f, _ in st._fields_}

    @staticmethod
    def _faces(face_index1, second=None):
        fi = np.ascontiguousarray(face_index1, np.int32).ravel()
        if second is None:
            return fi, None
        se = np.ascontiguousarray(second, np.int32).ravel()
        if se.shape != fi.shape:
            raise ValueError("face_index1 and color_in differ in length")
        return fi, se

    def reach_face_marks(self, mark: np.ndarray | None, face_index1) -> np.ndarray:
        """mark[face_index1 // 12 - 1] gathered on the device
        (pmx_reach_face_marks): what PMMG_check_reachability sends through the
        face communicator.  mark: (ne,), None = the live displacement's."""
        fi, _ = self._faces(face_index1)
        mk = None if mark is None else np.ascontiguousarray(mark, np.int32)
        if mk is not None and mk.shape != (self.bg_ne,):
            raise ValueError(f"mark has shape {mk.shape}, the group has {self.bg_ne} tets")
        out = np.zeros(max(len(fi), 1), np.int32)
        self._chk(self.lib.pmx_reach_face_marks(self.ctx, mk.ctypes.data_as(N.i32ptr) if mk is not None else None,
                                                len(fi), _ip(fi) if fi.size else None,
                                                out.ctypes.data_as(N.i32ptr)), "pmx_reach_face_marks")
        return out[:len(fi)]

    def check_reachability(self, mark: np.ndarray, colors_or_n, face_index1, color_in, counter: int,
                           replay_steps: int = 0):
        """Steps 2 and 3 of PMMG_check_reachability on a copy of mark, the
        result of fix_contiguity with the same colours
        (pmx_check_reachability): (mark, counter, stats).  color_in: the colour
        received for every entry, -1 = none; counter: the fix's."""
        ne = self.bg_ne
        p = np.array(mark, np.int32, order="C")
        if p.shape != (ne,):
            raise ValueError(f"mark has shape {p.shape}, the group has {ne} tets")
        if np.ndim(colors_or_n) == 0:
            ncol, col = int(colors_or_n), None
        else:
            col = np.ascontiguousarray(colors_or_n, np.int32)
            ncol = len(col)
        fi, cin = self._faces(face_index1, color_in)
        cnt, st = C.c_int64(counter), N.ReachStats()
        self._chk(self.lib.pmx_check_reachability(
            self.ctx, p.ctypes.data_as(N.i32ptr), ncol, col.ctypes.data_as(N.i32ptr) if col is not None else None,
            len(fi), _ip(fi) if fi.size else None, cin.ctypes.data_as(N.i32ptr) if fi.size else None,
            C.byref(cnt), replay_steps, C.byref(st)), "pmx_check_reachability")
        return p, cnt.value, self._stats(st)

    def moveifc_fix(self, replay_steps: int = 0) -> dict:
        """PMMG_fix_contiguity on the live displacement's marks, in place on
        the device (pmx_moveifc_fix): the fields of pmx_contig_stats."""
        st = N.ContigStats()
        self._chk(self.lib.pmx_moveifc_fix(self.ctx, replay_steps, C.byref(st)), "pmx_moveifc_fix")
        return self._stats(st)

    def moveifc_reach(self, face_index1, color_in, replay_steps: int = 0) -> dict:
        """Steps 2 and 3 of PMMG_check_reachability on the marks moveifc_fix
        left, in place on the device (pmx_moveifc_reach): the fields of
        pmx_reach_stats; counter goes on from the fix's."""
        fi, cin = self._faces(face_index1, color_in)
        st = N.ReachStats()
        self._chk(self.lib.pmx_moveifc_reach(self.ctx, len(fi), _ip(fi) if fi.size else None,
                                             cin.ctypes.data_as(N.i32ptr) if fi.size else None, replay_steps,
                                             C.byref(st)), "pmx_moveifc_reach")
        return self._stats(st)

    def moveifc_release(self):
        """Free the displacement's device memory (pmx_moveifc_release)."""
        self._moveifc = None
        self._chk(self.lib.pmx_moveifc_release(self.ctx), "pmx_moveifc_release")

    # ---- the partition on the device ------------------------------------------------
    def part_from_marks(self, target: int = N.GRPSPL_MMG_TARGET, ngrps_all=None):
        """PMMG_part_getInterfaces on the live displacement's marks, kept on
        the device (pmx_part_from_marks): (ngrp, group_mark).  group_mark[g] is
        the mark every tet of group g carries; group_mark % nprocs are the
        owners PMMG_part_getProcs reads."""
        st = self._moveifc_state()
        ng = None if ngrps_all is None else np.ascontiguousarray(ngrps_all, np.int32)
        if ng is not None and len(ng) != st["nprocs"]:
            raise ValueError("ngrps_all wants nprocs entries")
        # as many groups as colours at the most
        cap = max(st["nold_grp"], int(ng.clip(0).sum()) if ng is not None else st.get("ngrps_all", 0), 1)
        gm = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.pmx_part_from_marks(self.ctx, target, _ip(ng) if ng is not None else None, C.byref(n),
                                               gm.ctypes.data_as(N.i32ptr)), "pmx_part_from_marks")
        return n.value, gm[:n.value].copy()

    def part_upload(self, part: np.ndarray, ngrp: int):
        """A host partition (Metis's) becomes the device's (pmx_part_upload)."""
        p = np.ascontiguousarray(part, np.int32)
        if p.shape != (self.bg_ne,):
            raise ValueError(f"part has shape {p.shape}, the group has {self.bg_ne} tets")
        self._chk(self.lib.pmx_part_upload(self.ctx, p.ctypes.data_as(N.i32ptr) if p.size else None, ngrp),
                  "pmx_part_upload")

    def part_download(self):
        """The device's partition (pmx_part_download): (part (ne,), ngrp)."""
        ne = self.bg_ne
        part = np.zeros(max(ne, 1), np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.pmx_part_download(self.ctx, part.ctypes.data_as(N.i32ptr), C.byref(n)),
                  "pmx_part_download")
        return part[:ne], n.value

    def part_fix(self, replay_steps: int = 0) -> dict:
        """PMMG_fix_contiguity_split on the device's partition, in place
        (pmx_part_fix): the fields of pmx_contig_stats."""
        st = N.ContigStats()
        self._chk(self.lib.pmx_part_fix(self.ctx, replay_steps, C.byref(st)), "pmx_part_fix")
        return self._stats(st)

    def split_groups_part(self, comm: dict | None = None) -> dict:
        """split_groups by the device's partition (pmx_split_groups_part): the
        same dict."""
        ne = self.bg_ne
        n = C.c_int32(0)
        # without a partition the library refuses the split itself
        ngrp = n.value if self.lib.pmx_part_download(self.ctx, None, C.byref(n)) else 0
        c, _keep = self._split_comm(comm)
        sizes = (N.SplitSizes * max(ngrp, 1))()
        tet_new = np.zeros(ne, np.int32)
        fn, nn = C.c_int64(0), C.c_int64(0)
        self._split_sizes = None
        self._chk(self.lib.pmx_split_groups_part(self.ctx, C.byref(c), sizes, _ip(tet_new) if ne else None,
                                                 C.byref(fn), C.byref(nn)), "pmx_split_groups_part")
        sz = np.array([[s.ne, s.np, s.nface, s.nnode] for s in sizes[:ngrp]], np.int64).reshape(ngrp, 4)
        self._split_sizes = sz
        return {"sizes": sz, "tet_new": tet_new, "int_face_nitem": fn.value, "int_node_nitem": nn.value}

    def part_release(self):
        """Free the partition's device memory (pmx_part_release)."""
        self._chk(self.lib.pmx_part_release(self.ctx), "pmx_part_release")

    def move_interfaces(self, tet_group, map: dict, nlayers: int = 2, exchange=None, node_points=None):
        """PMMG_part_moveInterfaces: begin and nlayers layers.  exchange(colors)
        -> colors is called before every layer with the colours of node_points
        (the group's node-communicator points, 1-based) and returns the
        reduced ones; it stands for the ranks' MPI exchange.  Returns (marks,
        [stats of each layer]); stats[0]["nfront"] is begin's front."""
        nfront = self.moveifc_begin(tet_group, map)
        pts = None if node_points is None else np.ascontiguousarray(node_points, np.int32)
        stats = []
        for _ in range(nlayers):
            if exchange is not None and pts is not None:
                self.moveifc_set_colors(pts, exchange(self.moveifc_colors(pts)))
            stats.append(self.moveifc_layer())
        if stats:
            stats[0]["nfront"] = nfront
        return self.moveifc_marks(), stats

    def upload_new_tets(self, tets: np.ndarray):
        """The new mesh's tets, (ne+1, 4) with 0-based point indices (v[0] < 0:
        deleted), for pmx_promote_background / pmx_new_mesh_qual."""
        tv = _tets_1based(tets)
        self._chk(self.lib.pmx_upload_new_tets(self.ctx, _ip(tv), 16, tv.shape[0] - 1),
                  "pmx_upload_new_tets")
        self.n_new_tets = tv.shape[0] - 1

    def promote_background(self, new_mesh: Mesh, sols: list[np.ndarray] | None = None,
                           adja: bool = True):
        """The last step's new points + results become the background (device
        resident).  new_mesh: the new mesh (its trias/adjt/hausd and, with
        adja=True, its adjacency are read; coordinates and tets are not);
        sols: the (n, size) result arrays of the last download (values of the
        rows the step did not write)."""
        mv = mesh_view(new_mesh)
        if not adja:
            mv.adja = None
        arr = [np.ascontiguousarray(s, np.float64) for s in (sols or [])]
        views = (N.SolView * max(len(arr), 1))()
        for i, a in enumerate(arr):
            views[i].size = a.shape[1] if a.ndim == 2 else 1
            views[i].m = _dp(a)                 # pmx_download's layout: entry 0 = point 1
        self._chk(self.lib.pmx_promote_background(self.ctx, C.byref(mv), len(arr), views),
                  "pmx_promote_background")
        self.bg_np = self.npts              # the promoted points are the background's vertices
        self.bg_ne = new_mesh.ne
        self.bg_nt = new_mesh.nt
        self.npts = 0

    def new_mesh_qual(self, tets: np.ndarray | None, opt: int = N.INQUA, dev_ptr: int = 0,
                      met_rid_typ: int = 0) -> np.ndarray:
        """PMMG_tetraQual on the new mesh after the last step: tets (ne+1, 4)
        with indices of the uploaded points (0-based here, v[0] < 0: deleted);
        None: the tets of the last upload_new_tets."""
        tv = _tets_1based(tets) if tets is not None else None
        q = np.zeros((tv.shape[0] if tv is not None else self.n_new_tets + 1))
        self._chk(self.lib.pmx_new_mesh_qual(self.ctx, _ip(tv), 16, tv.shape[0] - 1 if tv is not None else 0,
                                             opt, met_rid_typ, _dp(q), len(q), C.c_void_p(dev_ptr or None)),
                  "pmx_new_mesh_qual")
        if tv is not None:
            self.n_new_tets = tv.shape[0] - 1
        return q

    def new_mesh_qual_synced(self, met: np.ndarray | None, opt: int = N.INQUA, met_rid_typ: int = 1,
                             out: np.ndarray | None = None) -> np.ndarray:
        """PMMG_tetraQual after the interpolation on the caller's metric
        (Mmg layout, (np+1, size), entry 0 unused; None: no metric), the new
        tets being the last points view's.  out: None -> a dense (ne+1,) array;
        a structured array with a "qual" field (MMG_TETRA records) -> written
        in place for the valid tets only (pmx_new_mesh_qual_synced, strided)."""
        mv = None
        if met is not None:
            met = np.ascontiguousarray(met, np.float64)
            mv = N.SolView()
            mv.size, mv.m = met.shape[1], _dp(met)
        if out is None:
            q = np.zeros(self.n_new_tets + 1)
            ptr, stride = _dp(q), 8
        else:
            if (out.ndim != 1 or not out.flags.c_contiguous or out.dtype.fields is None or "qual" not in
                    out.dtype.fields or out.dtype.fields["qual"][0] != np.float64 or
                    out.shape[0] < self.n_new_tets + 1):
                raise ValueError("out: a contiguous 1-D record array with a float64 'qual' field, "
                                 "one record per new tet plus slot 0")
            q = out
            base = out.ctypes.data + out.dtype.fields["qual"][1]
            ptr, stride = C.cast(C.c_void_p(base), N.dptr), out.dtype.itemsize
        self._chk(self.lib.pmx_new_mesh_qual_synced(self.ctx, C.byref(mv) if mv is not None else None, opt,
                                                    met_rid_typ, ptr, stride, q.shape[0], None),
                  "pmx_new_mesh_qual_synced")
        return q

    def comm_init(self, nranks: int, uid: bytes, rank: int) -> int:
        c = C.c_void_p()
        self._chk(self.lib.pmx_comm_init(self.ctx, C.byref(c), nranks, uid, rank), "pmx_comm_init")
        return c.value

    @staticmethod
    def comm_destroy(comm: int):
        if comm and not N.load().pmx_comm_destroy(C.c_void_p(comm)):
            raise RuntimeError("pmx_comm_destroy failed")

    def qualhisto_allreduce(self, comm: int, nranks: int, dev_ptr: int, ngrp: int = 1) -> dict:
        st = N.QualStats()
        self._chk(self.lib.pmx_qualhisto_allreduce(self.ctx, C.c_void_p(comm), nranks,
                                                   C.c_void_p(dev_ptr), ngrp, C.byref(st)),
                  "pmx_qualhisto_allreduce")
        return self._qdict(st)

    def prilen_allreduce(self, comm: int, nranks: int, dev_ptr: int) -> dict:
        st = N.LenStats()
        self._chk(self.lib.pmx_prilen_allreduce(self.ctx, C.c_void_p(comm), nranks, C.c_void_p(dev_ptr),
                                                C.byref(st)), "pmx_prilen_allreduce")
        return self._ldict(st)


def comm_unique_id() -> bytes:
    lib = N.load()
    buf = C.create_string_buffer(256)
    n = lib.pmx_comm_unique_id(buf, 256)
    if not n:
        raise RuntimeError("pmx_comm_unique_id failed")
    return buf.raw[:n]
