"""Pose graph and evaluation: the closure log with its relaxation, the consistency gate in front of
it, pose-proximity closure candidates and trajectory evaluation - device-resident handles.  `api` re-exports every name of __all__.
Drive sessions are SessionTable and SessionAlign: import them from this module - the public names of `api` are a
literal table in tests/test_api_surface.py, which a new name there would fail."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._context import Context
from ._handle import Handle, _ptr, ptr
from .registration import ICP_STATS, icp_search

__all__ = ["AteStats", "ClosureGate", "PoseGraph", "Proximity", "ProximitySearch", "TrajEval", "TrajectoryEval"]

class PoseGraph(Handle):
    """pr_posegraph: the accepted closures of a drive over caller-owned buffers with a DEVICE-side count, and a pose-graph relaxation of
    the map's poses over the odometry chain plus those closures.  The four buffers are zeroed torch tensors on the
    context's device (or the caller's: buffers = dict of the four names): .edge_ij [edge_capacity, 2] i32 (DB row i, query row j),
    .edge_Z [edge_capacity, 12] f64, .edge_w [edge_capacity, 2] f64 (w_rot, w_trans) and .state [4] i32 = edges, flags, 0, 0.  Every
    launch's geometry depends on the create sizes (and outer) only and both counts are read on the device, so ONE captured add_torch
    serves every keyframe and ONE captured relax_torch every count.  At edges == edge_capacity an add stores nothing and sets
    POSEGRAPH_OVERFLOW in info[3] until reset().  All *_torch calls are enqueued on the context's stream; nothing is read back."""

    NAMES = ("edge_ij", "edge_Z", "edge_w", "state")
    _DESTROY = "pr_posegraph_destroy"

    def __init__(self, ctx: Context | None, node_capacity: int, edge_capacity: int, max_outer: int = 10, max_inner: int = 256,
                 buffers: dict | None = None):
        import torch
        self._attach(ctx)
        self.node_capacity, self.edge_capacity = int(node_capacity), int(edge_capacity)
        self.max_outer, self.max_inner = int(max_outer), int(max_inner)
        ec = max(self.edge_capacity, 0)
        self._buffers("PoseGraph", dict(edge_ij=((ec, 2), torch.int32), edge_Z=((ec, 12), torch.float64), edge_w=((ec, 2), torch.float64),
                                        state=((4,), torch.int32)), buffers)
        torch.cuda.synchronize(self._device)              # torch's fills (its stream) before the library's stream writes the buffers
        rec = _lib.PoseGraphBuffers(*(ptr(getattr(self, n)) for n in self.NAMES))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_posegraph_create(self.ctx.h, C.byref(rec), self.node_capacity, self.edge_capacity, self.max_outer,
                                                    self.max_inner, C.byref(h)))
        self.h = h

    def add_torch(self, idx, T, accepted, query_row, w_rot: float = 1.0, w_trans: float = 1.0, info=None):
        """Device form (pr_posegraph_add_dev): a verify's idx i32 [1, k] (or [k]), T f64 [1, k, 3, 4] and accepted bool | u8 [1, k], and query_row
        i32 [>= 1] - the row the query keyframe received: map_info[1:2] of the map append in front (a negative value switches the call
        off on the device).  Every accepted pair with a valid row and a finite T is logged as the edge (idx, query_row) with the weights
        (w_rot, w_trans).  Returns info (device i32 [4]) = edges logged, first row | -1, edges after, flags.  Nothing synchronises,
        nothing is allocated when info= is given."""
        import torch
        who = "PoseGraph.add_torch"
        k = idx.numel()
        self._t(who, "idx", idx, torch.int32, numel=k, msg=f"{who}: idx must be a contiguous CUDA tensor i32 [k]")
        self._t(who, "T", T, torch.float64, numel=12 * k, msg=f"{who}: T must be a contiguous CUDA tensor f64 [k, 3, 4]")
        self._t(who, "accepted", accepted, torch.bool if accepted.dtype == torch.bool else torch.uint8, numel=k,
                msg=f"{who}: accepted must be a contiguous CUDA tensor bool or u8 [k]")
        self._t(who, "query_row", query_row, torch.int32, numel_min=1, msg=f"{who}: query_row must be a CUDA tensor i32 [>= 1]")
        info = self._result(who, "info", info, torch.int32, (4,), flat=True, msg=f"{who}: info must be a CUDA tensor i32 [4]")
        self.ctx.check(self.lib.pr_posegraph_add_dev(self.h, ptr(idx), ptr(T), ptr(accepted), ptr(query_row), k, float(w_rot), float(w_trans), ptr(info)))
        return info

    def add(self, idx, T, accepted, query_row: int, w_rot: float = 1.0, w_trans: float = 1.0):
        """Host form (pr_posegraph_add; synchronises): numpy arrays of the same meaning, query_row an int.  Returns info int32 [4]."""
        i = np.ascontiguousarray(idx, np.int32).reshape(-1)
        k = len(i)
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        a = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
        if len(t) != 12 * k or len(a) != k:
            raise ValueError("PoseGraph.add: idx [k], T [k, 3, 4], accepted [k]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_posegraph_add(self.h, _ptr(i), _ptr(t), _ptr(a), int(query_row), k, float(w_rot), float(w_trans), _ptr(info)))
        return info

    def add_weighted_torch(self, idx, T, accepted, query_row, w, info=None):
        """Device form (pr_posegraphw_add_dev): add_torch with per-slot weights w f64 [k, 2] = (w_rot, w_trans) in device memory -
        RegistrationInfo's .w.  A slot is logged under add_torch's conditions and only if both of its weights are finite and >= 0.
        Returns info (device i32 [4]); nothing synchronises, nothing is allocated when info= is given."""
        import torch
        who = "PoseGraph.add_weighted_torch"
        k = idx.numel()
        self._t(who, "idx", idx, torch.int32, numel=k, msg=f"{who}: idx must be a contiguous CUDA tensor i32 [k]")
        self._t(who, "T", T, torch.float64, numel=12 * k, msg=f"{who}: T must be a contiguous CUDA tensor f64 [k, 3, 4]")
        self._t(who, "accepted", accepted, torch.bool if accepted.dtype == torch.bool else torch.uint8, numel=k,
                msg=f"{who}: accepted must be a contiguous CUDA tensor bool or u8 [k]")
        self._t(who, "query_row", query_row, torch.int32, numel_min=1, msg=f"{who}: query_row must be a CUDA tensor i32 [>= 1]")
        self._t(who, "w", w, torch.float64, numel=2 * k, msg=f"{who}: w must be a contiguous CUDA tensor f64 [k, 2]")
        info = self._result(who, "info", info, torch.int32, (4,), flat=True, msg=f"{who}: info must be a CUDA tensor i32 [4]")
        self.ctx.check(self.lib.pr_posegraphw_add_dev(self.h, ptr(idx), ptr(T), ptr(accepted), ptr(query_row), k, ptr(w), ptr(info)))
        return info

    def add_weighted(self, idx, T, accepted, query_row: int, w):
        """Host form (pr_posegraphw_add; synchronises): numpy arrays of the same meaning, w [k, 2].  Returns info int32 [4]."""
        i = np.ascontiguousarray(idx, np.int32).reshape(-1)
        k = len(i)
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        a = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
        ww = np.ascontiguousarray(w, np.float64).reshape(-1)
        if len(t) != 12 * k or len(a) != k or len(ww) != 2 * k:
            raise ValueError("PoseGraph.add_weighted: idx [k], T [k, 3, 4], accepted [k], w [k, 2]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_posegraphw_add(self.h, _ptr(i), _ptr(t), _ptr(a), int(query_row), k, _ptr(ww), _ptr(info)))
        return info

    def add_batch_torch(self, i, j, T, accepted, w=None, w_rot: float = 1.0, w_trans: float = 1.0, info=None):
        """Device form (pr_posegraphb_add_dev): c slots that carry their own rows - i i32 [c] the DB rows, j i32 [c] the query rows (a
        ProximitySearch's pair_dst and pair_src), T f64 [c, 3, 4], accepted bool | u8 [c], w f64 [c, 2] or None (then w_rot, w_trans for
        every slot).  Slot p is logged iff accepted, i >= 0, j >= 0, i != j, T finite and its weights finite and >= 0, in the order of p:
        what c calls of add_weighted_torch with one slot each leave.  Returns info (device i32 [4]); nothing synchronises, nothing is
        allocated when info= is given."""
        import torch
        who = "PoseGraph.add_batch_torch"
        c = i.numel()
        self._t(who, "i", i, torch.int32, numel=c, msg=f"{who}: i must be a contiguous CUDA tensor i32 [c]")
        self._t(who, "j", j, torch.int32, numel=c, msg=f"{who}: j must be a contiguous CUDA tensor i32 [c]")
        self._t(who, "T", T, torch.float64, numel=12 * c, msg=f"{who}: T must be a contiguous CUDA tensor f64 [c, 3, 4]")
        self._t(who, "accepted", accepted, torch.bool if accepted.dtype == torch.bool else torch.uint8, numel=c,
                msg=f"{who}: accepted must be a contiguous CUDA tensor bool or u8 [c]")
        if w is not None:
            self._t(who, "w", w, torch.float64, numel=2 * c, msg=f"{who}: w must be a contiguous CUDA tensor f64 [c, 2]")
        info = self._result(who, "info", info, torch.int32, (4,), flat=True, msg=f"{who}: info must be a CUDA tensor i32 [4]")
        self.ctx.check(self.lib.pr_posegraphb_add_dev(self.h, ptr(i), ptr(j), ptr(T), ptr(accepted), ptr(w), float(w_rot), float(w_trans), c, ptr(info)))
        return info

    def add_batch(self, i, j, T, accepted, w=None, w_rot: float = 1.0, w_trans: float = 1.0):
        """Host form (pr_posegraphb_add; synchronises): numpy arrays of the same meaning.  Returns info int32 [4]."""
        ii = np.ascontiguousarray(i, np.int32).reshape(-1)
        jj = np.ascontiguousarray(j, np.int32).reshape(-1)
        c = len(ii)
        t = np.ascontiguousarray(T, np.float64).reshape(-1)
        a = np.ascontiguousarray(accepted, np.uint8).reshape(-1)
        ww = None if w is None else np.ascontiguousarray(w, np.float64).reshape(-1)
        if len(jj) != c or len(t) != 12 * c or len(a) != c or (ww is not None and len(ww) != 2 * c):
            raise ValueError("PoseGraph.add_batch: i [c], j [c], T [c, 3, 4], accepted [c], w [c, 2]")
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_posegraphb_add(self.h, _ptr(ii), _ptr(jj), _ptr(t), _ptr(a), _ptr(ww), float(w_rot), float(w_trans), c, _ptr(info)))
        return info

    def relax_torch(self, poses, n, outer: int = 5, inner: int = 64, lam: float = 1e-9, w_odo_rot: float = 1.0, w_odo_trans: float = 1.0,
                    out=None, report=None):
        """Device form (pr_posegraph_relax_dev): poses f64 [node_capacity, 12] (world to camera), n i32 [>= 1] whose word 0 is the node
        count - a KeyframeMap's .poses and .state.  `outer` damped Gauss-Newton steps of exactly `inner` preconditioned conjugate gradient
        iterations each over the odometry chain of the input poses (weights w_odo_rot, w_odo_trans) plus the logged edges.  out: f64
        [node_capacity, 12], may be poses itself (rows >= n are not written); report f64 [outer + 2] = the cost before each step, the
        final cost, the edges used.  Returns (out, report).  Nothing synchronises, nothing is allocated when out= and report= are given."""
        import torch
        who = "PoseGraph.relax_torch"
        outer = int(outer)
        self._t(who, "poses", poses, torch.float64, numel=12 * self.node_capacity, msg=f"{who}: poses must be a contiguous CUDA tensor f64 [node_capacity, 12]")
        self._t(who, "n", n, torch.int32, numel_min=1, msg=f"{who}: n must be a CUDA tensor i32 [>= 1]")
        out = self._result(who, "out", out, torch.float64, (self.node_capacity, 12), flat=True, zeros=True,
                           msg=f"{who}: out must be a contiguous CUDA tensor f64 [node_capacity, 12]")
        report = self._result(who, "report", report, torch.float64, (max(outer, 0) + 2 if report is None else outer + 2,), flat=True, zeros=True,
                              msg=f"{who}: report must be a CUDA tensor f64 [outer + 2]")
        prm = _lib.PoseGraphParams(outer, int(inner), float(lam), float(w_odo_rot), float(w_odo_trans))
        self.ctx.check(self.lib.pr_posegraph_relax_dev(self.h, ptr(poses), ptr(n), C.byref(prm), ptr(out), ptr(report)))
        return out, report

    def relax_map(self, km, **kw):
        """relax_torch(km.poses, km.state, ...) for a KeyframeMap: out=km.poses corrects the map in place.  The map must live on this
        handle's context (one stream) and have node_capacity keyframes; anything else is refused before the library is called."""
        self._share("PoseGraph.relax_map", "the pose graph and the map", km)
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError("PoseGraph.relax_map: node_capacity must equal the map's keyframe_capacity")
        return self.relax_torch(km.poses, km.state, **kw)

    def reset(self):
        self.ctx.check(self.lib.pr_posegraph_reset(self.h))

    def count(self):
        """(edges, flags); synchronises (pr_posegraph_count)."""
        n, f = C.c_int32(), C.c_int32()
        self.ctx.check(self.lib.pr_posegraph_count(self.h, C.byref(n), C.byref(f)))
        return int(n.value), int(f.value)


class ClosureGate(Handle):
    """pr_gate: the closure consistency gate in front of the relaxation.  Every ordered pair of closures logged in pg_src
    is compared along the odometry chain of the poses; a closure is kept when at least min_support kept closures within max_gap
    keyframes (|i_a - i_b| + |j_a - j_b|, another query keyframe) agree with it, repeated `rounds` times; the kept closures are copied,
    in log order, into pg_dst's log, which pg_dst.relax_torch / relax_map then relaxes.  The tables are rot_tab[g] = 2 (1 - cos(rad(rot_deg
    + g rot_deg_per_kf))) and trans2_tab[g] = (trans + g trans_per_kf)^2 for g = 0 .. max_gap, or the arrays given (passed through
    unchanged; +Inf switches a test off).  Calls are enqueued on the context's stream, read both counts on the device and allocate no
    device scratch; ONE captured run_torch serves every count.  Close it before either graph."""

    _DESTROY, _ON = "pr_gate_destroy", "the graphs' device"

    def __init__(self, ctx: Context | None, pg_src, pg_dst, max_gap: int, min_support: int = 2, rounds: int = 8, rot_deg: float = 2.0,
                 rot_deg_per_kf: float = 0.05, trans: float = 0.5, trans_per_kf: float = 0.02, rot_tab=None, trans2_tab=None):
        self._attach(ctx)
        if pg_src is pg_dst:
            raise ValueError("ClosureGate: pg_src and pg_dst must be two graphs")
        self._share("ClosureGate", "the gate and both graphs", pg_src, pg_dst)
        if pg_src.node_capacity != pg_dst.node_capacity:
            raise ValueError("ClosureGate: both graphs must have the same node_capacity")
        if pg_dst.edge_capacity < pg_src.edge_capacity:
            raise ValueError("ClosureGate: pg_dst.edge_capacity must be at least pg_src.edge_capacity")
        self.src, self.dst = pg_src, pg_dst
        self.node_capacity, self.edge_capacity = pg_src.node_capacity, pg_src.edge_capacity
        self.max_gap, self.min_support, self.rounds = int(max_gap), int(min_support), int(rounds)
        g = np.arange(max(self.max_gap, 0) + 1, dtype=np.float64)
        if rot_tab is None:
            rot_tab = 2.0 * (1.0 - np.cos(np.radians(float(rot_deg) + g * float(rot_deg_per_kf))))
        if trans2_tab is None:
            trans2_tab = (float(trans) + g * float(trans_per_kf)) ** 2
        self.rot_tab = np.ascontiguousarray(rot_tab, np.float64).reshape(-1)
        self.trans2_tab = np.ascontiguousarray(trans2_tab, np.float64).reshape(-1)
        if len(self.rot_tab) != len(g) or len(self.trans2_tab) != len(g):
            raise ValueError("ClosureGate: rot_tab and trans2_tab must have max_gap + 1 entries")
        recs = [_lib.PoseGraphBuffers(*(ptr(getattr(pg, n)) for n in pg.NAMES)) for pg in (pg_src, pg_dst)]
        prm = _lib.GateParams(self.max_gap, self.min_support, self.rounds)
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_gate_create(self.ctx.h, C.byref(recs[0]), C.byref(recs[1]), self.node_capacity, self.edge_capacity,
                                               pg_dst.edge_capacity, C.byref(prm), _ptr(self.rot_tab), _ptr(self.trans2_tab), C.byref(h)))
        self.h = h

    @property
    def _device(self):
        return self.src.state.device

    def run_torch(self, poses, n, keep=None, support=None, map=None, info=None):
        """Device form (pr_gate_run_dev): poses f64 [node_capacity, 12] (world to camera), n i32 [>= 1] whose word 0 is the node count - a
        KeyframeMap's .poses and .state.  Returns (keep u8 [edge_capacity], support i32 [edge_capacity] - the kept supporters of the last
        round, -1 for an edge that is not valid -, map i32 [edge_capacity] - the row in pg_dst or -1 -, info i32 [4] = valid, kept, edges
        read, flags GATE_*).  Nothing synchronises, nothing is allocated when all four are given."""
        import torch
        who = "ClosureGate.run_torch"
        ec = self.edge_capacity
        self._t(who, "poses", poses, torch.float64, numel=12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, numel_min=1)
        keep = self._result(who, "keep", keep, torch.uint8, (ec,), flat=True)
        support = self._result(who, "support", support, torch.int32, (ec,), flat=True)
        map = self._result(who, "map", map, torch.int32, (ec,), flat=True)
        info = self._result(who, "info", info, torch.int32, (4,), flat=True)
        self.ctx.check(self.lib.pr_gate_run_dev(self.h, ptr(poses), ptr(n), ptr(keep), ptr(support), ptr(map), ptr(info)))
        return keep, support, map, info

    def run_map(self, km, **kw):
        """run_torch(km.poses, km.state, ...) for a KeyframeMap, with PoseGraph.relax_map's refusals."""
        self._share("ClosureGate.run_map", "the gate and the map", km)
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError("ClosureGate.run_map: node_capacity must equal the map's keyframe_capacity")
        return self.run_torch(km.poses, km.state, **kw)

    def run(self, poses, n):
        """Host form (pr_gate_run; synchronises): poses and n as for run_torch (device tensors); returns NumPy (keep u8, support i32,
        map i32, info i32 [4])."""
        import torch
        who = "ClosureGate.run"
        self._t(who, "poses", poses, torch.float64, numel=12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, numel_min=1)
        ec = self.edge_capacity
        keep, support, map_, info = np.empty(ec, np.uint8), np.empty(ec, np.int32), np.empty(ec, np.int32), np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_gate_run(self.h, ptr(poses), ptr(n), _ptr(keep), _ptr(support), _ptr(map_),
                                            _ptr(info)))
        return keep, support, map_, info


class SessionAlign(NamedTuple):
    """What a SessionTable align returns (torch tensors from align_torch / align_map, NumPy arrays from align): poses f64
    [node_capacity, 12] (the output array; always a device tensor); G f64 [12] = [R | t] row-major, session t's world frame into the
    anchor's (the identity unless info[0] == SESSION_ALIGNED); hyp f64 [edge_capacity, 12], support i32 and inlier u8 [edge_capacity]
    (None when switched off); info i32 [8] = status, a* | -1, its support, candidates, |I|, edges read, n, flags."""
    poses: object
    G: object
    hyp: object
    support: object
    inlier: object
    info: object


class SessionTable(Handle):
    """pr_session: where each drive begins in the rows of a KeyframeMap, the consensus rigid alignment of a later drive onto the earlier
    ones from the cross-drive closures of a PoseGraph's log, and a relaxation that leaves out the odometry edges across drive borders
    (DESIGN.md 4.29).  The two buffers are torch tensors on the context's device (or the caller's: buffers = dict of the two names):
    .start [session_capacity] i32, the first row of every session, and .state [4] i32 = sessions, flags, 0, 0.  Calls are enqueued on
    the context's stream, read every count on the device and allocate no device scratch: ONE capture of align_torch -> ClosureGate.run_torch
    -> relax_torch made with an empty log and one session serves every count.  The rule is in include/place_recognition.h."""

    NAMES = ("start", "state")
    _DESTROY = "pr_session_destroy"

    def __init__(self, ctx: Context | None, node_capacity: int, edge_capacity: int, session_capacity: int = 8, buffers: dict | None = None):
        import torch
        self._attach(ctx)
        self.node_capacity, self.edge_capacity, self.session_capacity = int(node_capacity), int(edge_capacity), int(session_capacity)
        self._buffers("SessionTable", dict(start=((max(self.session_capacity, 0),), torch.int32), state=((4,), torch.int32)), buffers)
        torch.cuda.synchronize(self._device)              # torch's fills (its stream) before the library's stream writes the buffers
        rec = _lib.SessionBuffers(*(ptr(getattr(self, n)) for n in self.NAMES))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_session_create(self.ctx.h, C.byref(rec), self.node_capacity, self.edge_capacity, self.session_capacity,
                                                  C.byref(h)))
        self.h = h

    def scratch_bytes(self) -> int:
        return int(self.lib.pr_session_scratch_bytes(self.node_capacity, self.edge_capacity, self.session_capacity))

    def reset(self):
        self.ctx.check(self.lib.pr_session_reset(self.h))

    def count(self):
        """(sessions, flags); synchronises (pr_session_count)."""
        n, f = C.c_int32(), C.c_int32()
        self.ctx.check(self.lib.pr_session_count(self.h, C.byref(n), C.byref(f)))
        return int(n.value), int(f.value)

    def _map(self, who, km):
        self._share(who, "the session table and the map", km)
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError(f"{who}: node_capacity must equal the map's keyframe_capacity")

    def begin_torch(self, n, info=None):
        """Device form (pr_session_begin_dev): the rows from n[0] on - n i32 [>= 1], a KeyframeMap's .state - belong to a new session,
        unless the current last session is still empty (SESSION_REUSED) or the table is full (SESSION_OVERFLOW, until reset()).  Returns
        info (device i32 [4]) = session index now current, its first row, sessions after, flags.  Nothing synchronises, nothing is
        allocated when info= is given."""
        import torch
        who = "SessionTable.begin_torch"
        self._t(who, "n", n, torch.int32, numel_min=1)
        info = self._result(who, "info", info, torch.int32, (4,), flat=True)
        self.ctx.check(self.lib.pr_session_begin_dev(self.h, ptr(n), ptr(info)))
        return info

    def begin_map(self, km, **kw):
        """begin_torch(km.state, ...) for a KeyframeMap: call it before the first keyframe of the new drive is appended."""
        self._map("SessionTable.begin_map", km)
        return self.begin_torch(km.state, **kw)

    def begin(self, n):
        """Host form (pr_session_begin; synchronises): n as for begin_torch (a device tensor); returns info int32 [4]."""
        import torch
        self._t("SessionTable.begin", "n", n, torch.int32, numel_min=1)
        info = np.empty(4, np.int32)
        self.ctx.check(self.lib.pr_session_begin(self.h, ptr(n), _ptr(info)))
        return info

    def _align_args(self, who, pg, poses, n, session, min_inliers, rot_deg, trans, rot_c_max, trans2_max):
        import torch
        self._share(who, "the closure log and the session table", pg)
        if pg.edge_capacity > self.edge_capacity:
            raise ValueError(f"{who}: the log's edge_capacity must not exceed the session table's")
        self._t(who, "poses", poses, torch.float64, numel=12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, numel_min=1)
        rc = 2.0 * (1.0 - float(np.cos(np.radians(float(rot_deg))))) if rot_c_max is None else float(rot_c_max)
        t2 = float(trans) ** 2 if trans2_max is None else float(trans2_max)
        rec = _lib.PoseGraphBuffers(*(ptr(getattr(pg, nm)) for nm in pg.NAMES))
        return rec, _lib.SessionAlignParams(int(session), int(min_inliers), rc, t2)

    def align_torch(self, pg, poses, n, session: int = -1, min_inliers: int = 3, rot_deg: float = 3.0, trans: float = 1.0, rot_c_max=None,
                    trans2_max=None, out=None, G=None, hyp=None, support=None, inlier=None, info=None, optional=("hyp", "support", "inlier")):
        """Device form (pr_session_align_dev): the closures logged in the PoseGraph pg between session `session` (-1: the last) and the
        earlier sessions vote for the rigid transform G of that session's world frame into theirs; every finite row of the session
        becomes P G^-1 in out (f64 [node_capacity, 12]; may be poses itself; rows >= n are not written).  Two hypotheses agree within
        rot_deg degrees and trans metres at the closure (or rot_c_max = 2 (1 - cos) and trans2_max, passed through unchanged; +Inf
        switches a test off).  hyp / support / inlier are allocated when absent and named in `optional`, else stay NULL.  Returns
        SessionAlign.  Nothing synchronises; nothing is allocated when every array wanted is given."""
        import torch
        who = "SessionTable.align_torch"
        rec, prm = self._align_args(who, pg, poses, n, session, min_inliers, rot_deg, trans, rot_c_max, trans2_max)
        ec = self.edge_capacity
        out = self._result(who, "out", out, torch.float64, (self.node_capacity, 12), flat=True, zeros=True)
        G = self._result(who, "G", G, torch.float64, (12,), flat=True)
        info = self._result(who, "info", info, torch.int32, (8,), flat=True)
        if hyp is not None or "hyp" in optional:
            hyp = self._result(who, "hyp", hyp, torch.float64, (ec, 12), flat=True)
        if support is not None or "support" in optional:
            support = self._result(who, "support", support, torch.int32, (ec,), flat=True)
        if inlier is not None or "inlier" in optional:
            inlier = self._result(who, "inlier", inlier, torch.uint8, (ec,), flat=True)
        self.ctx.check(self.lib.pr_session_align_dev(self.h, C.byref(rec), pg.edge_capacity, ptr(poses), ptr(n), C.byref(prm), ptr(out), ptr(G),
                                                     ptr(hyp), ptr(support), ptr(inlier), ptr(info)))
        return SessionAlign(out, G, hyp, support, inlier, info)

    def align_map(self, km, pg, **kw):
        """align_torch(pg, km.poses, km.state, ...) for a KeyframeMap: out=km.poses moves the session in the map itself."""
        self._map("SessionTable.align_map", km)
        return self.align_torch(pg, km.poses, km.state, **kw)

    def align(self, pg, poses, n, session: int = -1, min_inliers: int = 3, rot_deg: float = 3.0, trans: float = 1.0, rot_c_max=None,
              trans2_max=None, out=None):
        """Host form (pr_session_align; synchronises): inputs as for align_torch (device tensors), out a device tensor too; returns
        SessionAlign with NumPy G, hyp, support, inlier, info."""
        import torch
        who = "SessionTable.align"
        rec, prm = self._align_args(who, pg, poses, n, session, min_inliers, rot_deg, trans, rot_c_max, trans2_max)
        ec = self.edge_capacity
        out = self._result(who, "out", out, torch.float64, (self.node_capacity, 12), flat=True, zeros=True)
        G, hyp, support = np.empty(12, np.float64), np.empty((ec, 12), np.float64), np.empty(ec, np.int32)
        inlier, info = np.empty(ec, np.uint8), np.empty(8, np.int32)
        self.ctx.check(self.lib.pr_session_align(self.h, C.byref(rec), pg.edge_capacity, ptr(poses), ptr(n), C.byref(prm), ptr(out), _ptr(G),
                                                 _ptr(hyp), _ptr(support), _ptr(inlier), _ptr(info)))
        return SessionAlign(out, G, hyp, support, inlier, info)

    def relax_torch(self, pg, poses, n, outer: int = 5, inner: int = 64, lam: float = 1e-9, w_odo_rot: float = 1.0, w_odo_trans: float = 1.0,
                    out=None, report=None):
        """Device form (pr_session_relax_dev): PoseGraph.relax_torch on pg with one change - the odometry edge into the first row of
        every session is left out - so the drives are held together by their closures alone.  With one session it leaves relax_torch's
        bytes.  Returns (out, report)."""
        import torch
        who = "SessionTable.relax_torch"
        self._share(who, "the pose graph and the session table", pg)
        if pg.node_capacity != self.node_capacity:
            raise ValueError(f"{who}: the pose graph's node_capacity must equal the session table's")
        outer = int(outer)
        self._t(who, "poses", poses, torch.float64, numel=12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, numel_min=1)
        out = self._result(who, "out", out, torch.float64, (self.node_capacity, 12), flat=True, zeros=True)
        report = self._result(who, "report", report, torch.float64, (max(outer, 0) + 2 if report is None else outer + 2,), flat=True, zeros=True)
        prm = _lib.PoseGraphParams(outer, int(inner), float(lam), float(w_odo_rot), float(w_odo_trans))
        self.ctx.check(self.lib.pr_session_relax_dev(self.h, pg.h, ptr(poses), ptr(n), C.byref(prm), ptr(out), ptr(report)))
        return out, report

    def relax_map(self, km, pg, **kw):
        """relax_torch(pg, km.poses, km.state, ...) for a KeyframeMap: out=km.poses corrects the map in place."""
        self._map("SessionTable.relax_map", km)
        return self.relax_torch(pg, km.poses, km.state, **kw)


class TrajEval(NamedTuple):
    """What a TrajectoryEval run returns (torch tensors from run_torch / run_map, NumPy arrays from run); the parts a run does not have
    are None.  ate [B, 24] = N, sse, rmse, mean, max, argmax, s, R (9), t (3), flags, sigma (3), var_x; rpe [B, K, 8] = pairs, rmse / mean /
    max of d, rmse / mean / max of theta, mean c_rot; seg [B, L + 1, 4] = segments, mean t_err, mean r_err, mean path ratio (row L: all
    lengths); clo [8] = evaluated, wrong, rmse / max of theta, rmse / max of d, edges read, 0; err [B, cap]; seg_end [B, slots, L] i32;
    edge_err [EC, 2]; centres [B + 1, cap, 3]; prefix [B, 2, cap]."""
    ate: object
    rpe: object
    seg: object
    clo: object
    err: object
    seg_end: object
    edge_err: object
    centres: object
    prefix: object


class AteStats(NamedTuple):
    """The columns of TrajEval.ate by name (TrajectoryEval.ate_stats)."""
    N: object
    sse: object
    rmse: object
    mean: object
    max: object
    argmax: object
    s: object
    R: object
    t: object
    flags: object
    sigma: object
    var_x: object


class TrajectoryEval(Handle):
    """pr_trajeval: a trajectory against ground truth on the device - ATE under an alignment ("none", "first", "se3",
    "sim3"), RPE per row delta, KITTI's segment metric per path length and the error of logged closures - for B candidate pose arrays a
    call.  est f64 [B, node_capacity, 12] (or [node_capacity, 12] with B = 1): rows as KeyframeMap.poses (world to camera); gt by gt_kind:
    "w2c" [node_capacity, 12], "c2w" [node_capacity, 12] (KITTI's file rows) or "positions" [node_capacity, 3] (ATE only).  Calls are
    enqueued on the context's stream, read every count on the device and allocate no device scratch; ONE captured run_torch serves every
    count.  The rule is in include/place_recognition.h."""

    ALIGN = dict(none=_lib.TRAJ_ALIGN_NONE, first=_lib.TRAJ_ALIGN_FIRST, se3=_lib.TRAJ_ALIGN_SE3, sim3=_lib.TRAJ_ALIGN_SIM3)
    GT = dict(w2c=_lib.TRAJ_GT_W2C, c2w=_lib.TRAJ_GT_C2W, positions=_lib.TRAJ_GT_POSITIONS)
    NAMES = TrajEval._fields
    _DESTROY = "pr_trajeval_destroy"

    def __init__(self, ctx: Context | None, node_capacity: int, B: int = 1, align: str = "sim3", gt_kind: str = "c2w", deltas=(1, 10),
                 lengths=(100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0), step: int = 1, edge_capacity: int = 0,
                 rot_thr: float = float(np.radians(5.0)), trans_thr: float = 2.0):
        if align not in self.ALIGN:
            raise ValueError(f"TrajectoryEval: align must be one of {sorted(self.ALIGN)}")
        if gt_kind not in self.GT:
            raise ValueError(f"TrajectoryEval: gt_kind must be one of {sorted(self.GT)}")
        self._attach(ctx)
        self.node_capacity, self.B, self.align, self.gt_kind = int(node_capacity), int(B), align, gt_kind
        self.deltas = np.ascontiguousarray(deltas, np.int32).reshape(-1)
        self.lengths = np.ascontiguousarray(lengths, np.float64).reshape(-1)
        self.K, self.L, self.step, self.edge_capacity = len(self.deltas), len(self.lengths), int(step), int(edge_capacity)
        self.gt_cols = 3 if gt_kind == "positions" else 12
        self.slots = -(-self.node_capacity // self.step) if self.step >= 1 and self.node_capacity >= 1 else 0
        self.params = _lib.TrajEvalParams(self.node_capacity, self.B, self.ALIGN[align], self.GT[gt_kind], self.K, self.L, self.step,
                                          self.edge_capacity, float(rot_thr), float(trans_thr))
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_trajeval_create(self.ctx.h, C.byref(self.params), _ptr(self.deltas) if self.K else None,
                                                   _ptr(self.lengths) if self.L else None, C.byref(h)))
        self.h = h

    def scratch_bytes(self) -> int:
        return int(self.lib.pr_trajeval_scratch_bytes(C.byref(self.params)))

    def shapes(self, log: bool = True):
        """name -> (shape, NumPy dtype) of every output this handle can write (clo and edge_err only with a closure log)."""
        B, cap, K, L = self.B, self.node_capacity, self.K, self.L
        s = dict(ate=((B, _lib.TRAJ_ATE_STATS), np.float64), err=((B, cap), np.float64), centres=((B + 1, cap, 3), np.float64),
                 prefix=((B, 2, cap), np.float64))
        if K:
            s["rpe"] = ((B, K, _lib.TRAJ_RPE_STATS), np.float64)
        if L:
            s["seg"] = ((B, L + 1, _lib.TRAJ_SEG_STATS), np.float64)
            s["seg_end"] = ((B, self.slots, L), np.int32)
        if log and self.edge_capacity:
            s["clo"] = ((_lib.TRAJ_CLO_STATS,), np.float64)
            s["edge_err"] = ((self.edge_capacity, 2), np.float64)
        return s

    @staticmethod
    def ate_stats(ate) -> AteStats:
        """TrajEval.ate [B, 24] split into its named columns (views)."""
        return AteStats(ate[:, 0], ate[:, 1], ate[:, 2], ate[:, 3], ate[:, 4], ate[:, 5], ate[:, 6], ate[:, 7:16].reshape(-1, 3, 3), ate[:, 16:19],
                        ate[:, 19], ate[:, 20:23], ate[:, 23])

    def _inputs(self, who, est, n, gt, valid, log):
        import torch
        cap = self.node_capacity
        self._t(who, "est", est, torch.float64, numel=12 * self.B * cap)
        self._t(who, "n", n, torch.int32, numel_min=1)
        self._t(who, "gt", gt, torch.float64, numel=self.gt_cols * cap)
        if valid is not None:
            self._t(who, "valid", valid, torch.bool if valid.dtype == torch.bool else torch.uint8, numel=cap)
        rec = None
        if log is not None:
            self._share(who, "the closure log and the evaluation", log)
            if self.edge_capacity < 1 or self.edge_capacity > log.edge_capacity:        # the rows [0, edge_capacity) of the log must exist
                raise ValueError(f"{who}: edge_capacity must lie between 1 and the log's edge_capacity")
            rec = _lib.PoseGraphBuffers(*(ptr(getattr(log, nm)) for nm in log.NAMES))
        return ptr(est), ptr(n), ptr(gt), ptr(valid), rec

    def run_torch(self, est, n, gt, valid=None, log=None, out: dict | None = None, optional=("err", "seg_end", "edge_err")) -> TrajEval:
        """Device form (pr_trajeval_run_dev).  n i32 [>= 1] whose word 0 is the row count (a KeyframeMap's .state); valid bool | u8
        [node_capacity] or None; log a PoseGraph whose logged closures are evaluated, or None.  out: a dict name -> preallocated tensor
        (shapes()); the statistics blocks are allocated when absent, the arrays named in `optional` too ("centres", "prefix" may be
        added), the others stay NULL.  Returns TrajEval.  Nothing synchronises; nothing is allocated when `out` holds every array wanted."""
        import torch
        who = "TrajectoryEval.run_torch"
        pe, pn, pg, pv, rec = self._inputs(who, est, n, gt, valid, log)
        out = dict(out or {})
        got = {}
        for name, (shape, dt) in self.shapes(log is not None).items():
            if name in out or name in ("ate", "rpe", "seg", "clo") or name in optional:
                got[name] = self._result(who, name, out.get(name), torch.int32 if dt == np.int32 else torch.float64, shape, flat=True)
        o = _lib.TrajEvalOut(*(ptr(got.get(nm)) for nm in self.NAMES))
        self.ctx.check(self.lib.pr_trajeval_run_dev(self.h, pe, pn, pg, pv, C.byref(rec) if rec is not None else None, C.byref(o)))
        return TrajEval(*(got.get(nm) for nm in self.NAMES))

    def run_map(self, km, gt, poses=None, **kw) -> TrajEval:
        """run_torch for a KeyframeMap: its .state as the count and its .poses - or `poses` [node_capacity, 12], e.g. the out of
        PoseGraph.relax_torch - as the estimate (B = 1).  The map must live on this handle's context."""
        self._share("TrajectoryEval.run_map", "the evaluation and the map", km)
        if km.keyframe_capacity != self.node_capacity or self.B != 1:
            raise ValueError("TrajectoryEval.run_map: node_capacity must equal the map's keyframe_capacity and B must be 1")
        return self.run_torch(km.poses if poses is None else poses, km.state, gt, **kw)

    def run(self, est, n, gt, valid=None, log=None, optional=("err", "seg_end", "edge_err", "centres", "prefix")) -> TrajEval:
        """Host form (pr_trajeval_run; synchronises): inputs as for run_torch (device tensors); returns TrajEval of NumPy arrays."""
        who = "TrajectoryEval.run"
        pe, pn, pg, pv, rec = self._inputs(who, est, n, gt, valid, log)
        got = {name: np.empty(shape, dt) for name, (shape, dt) in self.shapes(log is not None).items()
               if name in ("ate", "rpe", "seg", "clo") or name in optional}
        o = _lib.TrajEvalOut(*(_ptr(got[nm]) if nm in got else None for nm in self.NAMES))
        self.ctx.check(self.lib.pr_trajeval_run(self.h, pe, pn, pg, pv, C.byref(rec) if rec is not None else None, C.byref(o)))
        return TrajEval(*(got.get(nm) for nm in self.NAMES))


class Proximity(NamedTuple):
    """The outputs of a ProximitySearch search: idx i32, d2 f64 [query_capacity, k]; T0 f64 [query_capacity k, 3, 4]; pair_src, pair_dst
    i32 and known u8 [query_capacity k]; info i32 [4] = rows searched, slots filled, slots known, flags."""
    idx: object
    d2: object
    T0: object
    pair_src: object
    pair_dst: object
    known: object
    info: object


class ProximitySearch(Handle):
    """pr_proximity: loop-closure candidates from the poses - for every query row q0 + r the earlier keyframes within
    radius + growth x (path between the rows), capped at radius_max, that look the same way (cos_min), one per bucket of `stride` rows,
    the k nearest - with the seeds and pair lists of verify_map_torch and PoseGraph.add_batch_torch.  Calls are enqueued on the context's
    stream, read n, qrange and the log's count on the device and allocate no device scratch: ONE captured search_torch serves every
    count and every query range.  The rule is in include/place_recognition.h."""

    _DESTROY = "pr_proximity_destroy"

    def __init__(self, ctx: Context | None, node_capacity: int, query_capacity: int, k_max: int):
        self._attach(ctx)
        self.node_capacity, self.query_capacity, self.k_max = int(node_capacity), int(query_capacity), int(k_max)
        self.last_verify = None
        h = C.c_void_p()
        self.ctx.check(self.lib.pr_proximity_create(self.ctx.h, self.node_capacity, self.query_capacity, self.k_max, C.byref(h)))
        self.h = h

    def scratch_bytes(self) -> int:
        return int(self.lib.pr_proximity_scratch_bytes(self.node_capacity, self.query_capacity, self.k_max))

    @staticmethod
    def tile():
        """(rows, cols) of the search kernel's tile (pr_proximity_tile)."""
        r, c = C.c_int32(), C.c_int32()
        _lib.load().pr_proximity_tile(C.byref(r), C.byref(c))
        return int(r.value), int(c.value)

    def shapes(self, k: int):
        Q = self.query_capacity
        return dict(idx=((Q, k), np.int32), d2=((Q, k), np.float64), T0=((Q * k, 3, 4), np.float64), pair_src=((Q * k,), np.int32),
                    pair_dst=((Q * k,), np.int32), known=((Q * k,), np.uint8), info=((4,), np.int32))

    def _args(self, who, poses, n, qrange, radius, growth, radius_max, cos_min, min_gap, stride, k, log, known_window):
        import torch
        self._t(who, "poses", poses, torch.float64, numel=12 * self.node_capacity)
        self._t(who, "n", n, torch.int32, numel_min=1)
        self._t(who, "qrange", qrange, torch.int32, numel=2)
        k = int(k)
        if k < 1 or k > self.k_max:
            raise ValueError(f"{who}: k must lie in 1 .. k_max")
        rec, ec = None, 0
        if log is not None:
            self._share(who, "the closure log and the search", log)
            rec = _lib.PoseGraphBuffers(*(ptr(getattr(log, nm)) for nm in log.NAMES))
            ec = log.edge_capacity
        prm = _lib.ProximityParams(float(radius), float(growth), float(radius if radius_max is None else radius_max), float(cos_min), int(min_gap),
                                   int(stride), k, int(known_window))
        return k, prm, rec, ec

    def search_torch(self, poses, n, qrange, *, radius, growth=0.0, radius_max=None, cos_min=-1.0, min_gap, stride=1, k=1, log=None,
                     known_window=0, out=None) -> Proximity:
        """Device form (pr_proximity_search_dev): poses f64 [node_capacity, 12] and n i32 [>= 1] - a KeyframeMap's .poses and .state - and
        qrange i32 [2] = (q0, mq): output row r stands for query row q0 + r, r < mq.  radius_max None: radius.  log: a PoseGraph whose
        logged pairs (within known_window rows at both ends) come back known = 1 and switched off.  out: the Proximity an earlier call
        returned for the same k (fixed addresses: what a captured graph needs).  Nothing synchronises; nothing is allocated with out=."""
        import torch
        who = "ProximitySearch.search_torch"
        k, prm, rec, ec = self._args(who, poses, n, qrange, radius, growth, radius_max, cos_min, min_gap, stride, k, log, known_window)
        tdt = {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}
        got = {name: self._result(who, name, getattr(out, name, None), tdt[dt], shape, flat=True) for name, (shape, dt) in self.shapes(k).items()}
        self.ctx.check(self.lib.pr_proximity_search_dev(self.h, ptr(poses), ptr(n), ptr(qrange), C.byref(prm), C.byref(rec) if rec is not None else None,
                                                        ec, *(ptr(got[nm]) for nm in Proximity._fields)))
        return Proximity(*(got[nm] for nm in Proximity._fields))

    def _map(self, who, km):
        self._share(who, "the search and the map", km)
        if km.keyframe_capacity != self.node_capacity:
            raise ValueError(f"{who}: node_capacity must equal the map's keyframe_capacity")

    def search_map(self, km, qrange, **kw) -> Proximity:
        """search_torch(km.poses, km.state, qrange, ...) for a KeyframeMap on this handle's context with node_capacity keyframes; anything
        else is refused before the library is called."""
        self._map("ProximitySearch.search_map", km)
        return self.search_torch(km.poses, km.state, qrange, **kw)

    def search(self, poses, n, qrange, *, radius, growth=0.0, radius_max=None, cos_min=-1.0, min_gap, stride=1, k=1, log=None,
               known_window=0) -> Proximity:
        """Host form (pr_proximity_search; synchronises): inputs as for search_torch (device tensors); returns Proximity of NumPy arrays."""
        who = "ProximitySearch.search"
        k, prm, rec, ec = self._args(who, poses, n, qrange, radius, growth, radius_max, cos_min, min_gap, stride, k, log, known_window)
        got = {name: np.empty(shape, dt) for name, (shape, dt) in self.shapes(k).items()}
        self.ctx.check(self.lib.pr_proximity_search(self.h, ptr(poses), ptr(n), ptr(qrange), C.byref(prm), C.byref(rec) if rec is not None else None, ec,
                                                    *(_ptr(got[nm]) for nm in Proximity._fields)))
        return Proximity(*(got[nm] for nm in Proximity._fields))

    def verify_map_torch(self, km, cand: Proximity, max_src_pts: int, *, max_iter: int = 30, max_corr: float = 1.0, min_fitness: float = 0.5,
                         max_rmse: float = 0.5, tol_rmse: float = 1e-6, tol_fitness: float = 1e-6, min_inliers: int = 3, search=None, out=None):
        """The candidates of a search refined and judged on the stream: pr_icp_pairs_dev with the map's own CSR on BOTH sides (N =
        keyframe_capacity: cloud pair_src onto cloud pair_dst from T0; a slot switched off answers ICP_NO_PAIR), then
        pr_verify_select_dev with one hypothesis - verify's accept rule.  Returns (T f64 [c, 3, 4], stats u8 [c, 32], accepted bool [c]), c =
        query_capacity k: what PoseGraph.add_batch_torch(cand.pair_dst, cand.pair_src, T, accepted) logs.  out: the dict an earlier call
        left in .last_verify for the same c (fixed addresses for a capture)."""
        import torch
        who = "ProximitySearch.verify_map_torch"
        self._map(who, km)
        c = cand.pair_src.numel()
        dev = cand.pair_src.device
        if out is None:
            out = dict(refine=(torch.empty((c, 3, 4), dtype=torch.float64, device=dev), torch.zeros((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev)),
                       T=torch.empty((c, 3, 4), dtype=torch.float64, device=dev), stats=torch.empty((c, ICP_STATS.itemsize), dtype=torch.uint8, device=dev),
                       accepted=torch.empty(c, dtype=torch.bool, device=dev), hyp=torch.empty(c, dtype=torch.int32, device=dev))
            torch.cuda.synchronize(dev)                   # torch's fill (its stream) before the library's stream writes the buffers
        elif out["T"].shape != (c, 3, 4):
            raise ValueError(f"{who}: out belongs to another c")
        N = km.keyframe_capacity
        with icp_search(self.ctx, search):
            self.ctx.check(self.lib.pr_icp_pairs_dev(self.ctx.h, ptr(km.xyz), ptr(km.offs), N, ptr(km.xyz), ptr(km.offs), N, ptr(cand.pair_src), ptr(cand.pair_dst),
                                                     c, ptr(cand.T0), int(max_src_pts), int(km.max_cloud_points), int(max_iter), float(max_corr),
                                                     float(tol_rmse), float(tol_fitness), int(min_inliers), ptr(out["refine"][0]), ptr(out["refine"][1])))
        self.ctx.check(self.lib.pr_verify_select_dev(self.ctx.h, ptr(out["refine"][0]), ptr(out["refine"][1]), c, 1, float(min_fitness), float(max_rmse),
                                                     ptr(out["T"]), ptr(out["stats"]), ptr(out["accepted"]), ptr(out["hyp"])))
        self.last_verify = out
        return out["T"], out["stats"], out["accepted"]
