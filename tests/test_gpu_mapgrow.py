"""The incremental world map on the device (pr_mapgrow, mapgrow.hip).  The contract is the rebuild's bytes: after EVERY
extend + normals the five world arrays, state and the two normal arrays are compared byte for byte with a rebuild (fuse -> index ->
normals) on a SECOND set of handles over the same map and with the restatement (mapgrow_np.py); the index is compared as a map through
pr_maploc_count, pr_maploc_nn_dev and the two refines, bit for bit, with an exclusion window over the newest rows.  Guard words sit behind
all five world arrays, both normal arrays and every info."""
import ctypes as C

import numpy as np
import pytest
import torch

import mapgrow_np as gnp
import maploc_np as mnp
import worldmap_np as wnp
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_map import KCAP, MAXC, PCAP, dev, pose_inputs, same_bytes, seq07  # noqa: F401  (seq07: the drive's fixture)
from test_gpu_maploc import GUARD, I32, guarded

pytestmark = pytest.mark.gpu

WORLD = dict(xyz=(3, torch.float64), inten=(1, torch.float32), src=(1, torch.int64), row=(1, torch.int32), count=(1, torch.int32))
KW = dict(max_iter=6, max_corr=0.45, tol_rmse=1e-9, tol_fitness=1e-9)


class Side:
    """a world map over guarded buffers, a localiser, a plane localiser and a guarded normal pair over one map"""

    def __init__(self, ctx, km, ocap, cell, max_src):
        self.guards, bufs = [], {}
        for n, (w, dt) in WORLD.items():
            t, g = guarded((ocap, w) if w > 1 else (ocap,), dt)
            t.zero_()
            bufs[n] = t
            self.guards.append(g)
        bufs["state"] = torch.zeros(4, dtype=torch.int32, device="cuda")
        self.wm = api.WorldMap(ctx, km, ocap, buffers=bufs)
        self.ml = api.MapLocalizer(ctx, self.wm, cell, 2, max_src)
        self.pl = api.PlaneLocalizer(ctx, self.ml)
        (self.nrm, g1), (self.ninfo, g2) = guarded((ocap, 3), torch.float64), guarded((ocap,), torch.int32)
        self.nrm.zero_(); self.ninfo.zero_()
        self.guards += [g1, g2]
        torch.cuda.synchronize()

    def intact(self):
        for g in self.guards:
            g()

    def host(self):
        d = {n: getattr(self.wm, n).cpu().numpy() for n in api.WorldMap.NAMES}
        d["normals"], d["ninfo"] = self.nrm.cpu().numpy(), self.ninfo.cpu().numpy()
        return d

    def close(self):
        self.pl.close(); self.ml.close(); self.wm.close()


class Rig:
    """one map; side A grows (a MapGrower over it), side B is rebuilt for every comparison; M is the restatement beside A"""

    def __init__(self, ctx, kcap, pcap, mcp, ocap, cell, nkw=gnp.NORMALS, max_src=600, model=True):
        self.ctx, self.ocap, self.cell, self.nkw, self.mcp, self.kcap = ctx, ocap, cell, nkw, mcp, kcap
        self.km = api.KeyframeMap(ctx, kcap, pcap, mcp)
        self.A, self.B = Side(ctx, self.km, ocap, cell, max_src), Side(ctx, self.km, ocap, cell, max_src)
        self.mg = api.MapGrower(ctx, self.A.wm, self.A.ml)
        self.M = gnp.Model(np.zeros((pcap, 3)), np.zeros(pcap, np.float32), np.zeros(kcap + 1, np.int64), ocap, cell, mcp) if model else None
        (self.info, self.ginfo) = guarded((4,), torch.int64)

    def append(self, cam, inten=None, pose=None, id_=0):
        cam = np.asarray(cam, np.float64).reshape(-1, 3)
        inten = np.linspace(0, 1, len(cam)).astype(np.float32) if inten is None else inten
        pose = wnp.identity_poses(1)[0] if pose is None else pose
        return self.km.append(cam, inten, [0, len(cam)], np.zeros((1, 16)), poses=np.asarray(pose).reshape(1, 12), ids=[id_])

    def map_host(self):
        torch.cuda.synchronize()
        return (self.km.xyz.cpu().numpy(), self.km.inten.cpu().numpy(), self.km.offs.cpu().numpy(), self.km.poses.cpu().numpy(),
                int(self.km.state.cpu().numpy()[0]))

    def _model_map(self):
        self.M.m_xyz, self.M.m_inten, self.M.m_offs, poses, n = self.map_host()
        return poses, n

    def rebuild(self, n=None, poses=None):
        """the rebuild on side A through MapGrower.rebuild_torch (fuse -> index -> normals -> sync), and on the model"""
        self.mg.rebuild_torch(self.A.pl, None if poses is None else dev(poses), None if n is None else I32(n), out=(self.A.nrm, self.A.ninfo),
                              **self.nkw)
        torch.cuda.synchronize()
        if self.M is not None:
            mp_, mn = self._model_map()
            self.M.rebuild(mp_ if poses is None else poses, mn if n is None else n, self.nkw)

    def extend(self, row, poses=None, normals=True):
        """extend + normals on side A and on the model; -> info (host)"""
        self.info.fill_(GUARD)
        self.mg.extend_torch(I32(row), None if poses is None else dev(poses), info=self.info)
        if normals:
            self.mg.normals_torch(self.nkw["radius"], self.nkw["min_nbrs"], self.nkw["max_ratio"], self.A.nrm, self.A.ninfo)
        torch.cuda.synchronize()
        self.ginfo(); self.A.intact()
        info = self.info.cpu().numpy().copy()
        if self.M is not None:
            mp_, mn = self._model_map()
            want = self.M.extend(mp_ if poses is None else poses, row, mn)
            assert info.tolist() == want.tolist(), ("info against the restatement", row, info, want)
            if normals:
                self.M.normals(**self.nkw)
        return info

    def check(self, n, what, poses=None, searches=True):
        """side A against a rebuild at the count n on side B, and against the model"""
        B, A = self.B, self.A
        pt = None if poses is None else dev(poses)
        B.wm.fuse_torch(pt, I32(n), self.cell, 1, "first")
        B.ml.index_torch()
        B.pl.normals_torch(out=(B.nrm, B.ninfo), **self.nkw)
        torch.cuda.synchronize()
        A.intact(); B.intact()
        a, b = A.host(), B.host()
        R = int(b["state"][0])
        assert a["state"].tobytes() == b["state"].tobytes(), (what, a["state"], b["state"])
        for name in WORLD:
            assert same_bytes(a[name][:R], b[name][:R]), (what, name, np.flatnonzero((a[name][:R] != b[name][:R]).reshape(R, -1).any(axis=1))[:8])
        assert a["ninfo"].tolist() == b["ninfo"].tolist(), (what, np.flatnonzero(a["ninfo"] != b["ninfo"])[:8])
        assert same_bytes(a["normals"], b["normals"]), (what, "normals")
        assert A.ml.count() == B.ml.count(), (what, A.ml.count(), B.ml.count())
        assert self.mg.count()[:2] == (n, R), (what, self.mg.count())
        if self.M is not None:
            M = self.M
            assert M.state.tobytes() == a["state"].tobytes(), (what, "model state", M.state, a["state"])
            for name in WORLD:
                assert same_bytes(getattr(M, name)[:R], a[name][:R]), (what, "model", name)
            assert M.ninfo.tolist() == a["ninfo"].tolist() and same_bytes(M.normals_, a["normals"]), (what, "model normals")
            assert M.first == mnp.index(a["xyz"], R, self.cell, self.ocap)["first"], (what, "model index")
        if searches and R:
            self.searches(a, R, what)
        return a, R

    def searches(self, a, R, what):
        """pr_maploc_nn_dev, pr_maploc_refine_dev and pr_mapplane_refine_dev through A's grown index and B's fresh one: bit for bit"""
        rng = np.random.default_rng(R)
        pick = rng.permutation(R)[:500]
        xq = a["xyz"][pick] + rng.normal(0, 0.12 * self.cell, (len(pick), 3))
        newest = int(a["row"][:R].max())
        T = np.stack([np.hstack([np.eye(3), np.zeros((3, 1))])] * 2)
        T[1, :, 3] = (0.02, -0.03, 0.01)
        args = (dev(xq), dev([0, len(xq)], np.int64), dev([0, 0], np.int32), dev(T))
        excl = dev([[newest, newest], [1, 0]], np.int32)
        out = []
        for S in (self.A, self.B):
            oo, ji, dd = S.ml.nn_torch(*args, excl, self.nkw["radius"])
            rT, rs = S.ml.refine_torch(*args, excl, min_inliers=3, **KW)
            pT, ps = S.pl.refine_torch(*args, S.nrm, S.ninfo, excl, min_inliers=6, **KW)
            torch.cuda.synchronize()
            total = int(oo[-1])
            out.append([t.cpu().numpy() for t in (oo, ji[:total], dd[:total], rT, rs, pT, ps)])
        for x, y, name in zip(out[0], out[1], ("nn offs", "nn idx", "nn d2", "refine T", "refine stats", "plane T", "plane stats")):
            assert x.tobytes() == y.tobytes(), (what, name)
        j0 = out[0][1][out[0][0][0]:out[0][0][1]]                       # pair 0: the newest keyframe's rows are excluded
        assert (out[0][1] >= 0).any() and not (a["row"][j0[j0 >= 0]] == newest).any(), (what, "the window")

    def close(self):
        self.mg.close(); self.A.close(); self.B.close(); self.km.close()


# ------------------------------------------------------------------------------------------------ 1. the launch geometry's edges
def cells_cloud(cells, per, rng, cell=1.0):
    """`per` points in each of the voxels `cells`, in one shuffled cloud"""
    c = np.repeat(np.asarray(cells, np.float64), per, axis=0)
    return (c[rng.permutation(len(c))] + 0.1 + 0.8 * rng.random((len(c), 3))) * cell


@pytest.mark.parametrize("ocap", (32, 600))
def test_keyframes_at_the_geometry_edges(ocap):
    """clouds of 0, 1, 255, 256, 257 and 513 points and an empty row in between, at tables of 64 and 2048 slots"""
    assert 1 << mnp.log2T(ocap) == (64 if ocap == 32 else 2048)
    rng = np.random.default_rng(ocap)
    ctx = _stream_context(0)
    W = Rig(ctx, 10, 4096, 513, ocap, 1.0, nkw=dict(radius=0.99, min_nbrs=4, max_ratio=0.3))
    W.rebuild()
    W.check(0, "the empty map", searches=False)
    if ocap == 32:                                                   # 28 voxels among them the ten whose chain wraps the table's end
        pool = np.array(mnp.COLLIDING_CELLS[:28], np.float64)
        draw = lambda s: cells_cloud(pool[rng.integers(0, len(pool), max(s, 1))][:s], 1, rng) if s else np.zeros((0, 3))
    else:                                                            # a floor and a wall of voxels: fewer than 600 of them
        pool = np.array([(a, b, 0) for a in range(16) for b in range(16)] + [(0, b, c) for b in range(16) for c in range(1, 16)], np.float64)
        draw = lambda s: cells_cloud(pool[rng.integers(0, len(pool), max(s, 1))][:s], 1, rng) if s else np.zeros((0, 3))
    for r, s in enumerate((0, 1, 255, 0, 256, 257, 513)):
        ainfo = W.append(draw(s))
        assert ainfo[1] == r
        info = W.extend(int(ainfo[1]))
        assert info[2] == s and info[3] == 0, (r, info)
        W.check(r + 1, (ocap, "size", s))
    assert W.mg.count() == (7, int(W.A.wm.state[0]), 0)
    W.close(); ctx.close()


def test_one_voxel_own_voxels_known_voxels_and_a_flipping_normal():
    rng = np.random.default_rng(2)
    ctx = _stream_context(0)
    W = Rig(ctx, 8, 4096, 600, 1024, 1.0, nkw=dict(radius=0.99, min_nbrs=4, max_ratio=0.5))
    W.rebuild()
    one = cells_cloud([(3, 3, 3)], 513, rng)                         # 513 points in ONE new voxel: one row, count 513
    assert W.extend(int(W.append(one)[1])).tolist() == [1, 1, 513, 0]
    a, R = W.check(1, "one voxel")
    assert R == 1 and a["count"][0] == 513 and a["src"][0] == 0
    own = cells_cloud([(a, b, 7) for a in range(20) for b in range(20)], 1, rng)     # every point in its own voxel
    assert W.extend(int(W.append(own)[1])).tolist() == [400, 401, 400, 0]
    a, R = W.check(2, "own voxels")
    assert (a["count"][1:401] == 1).all() and (a["ninfo"][1:401] > 0).any()
    known = cells_cloud([(3, 3, 3)] * 5 + [(a, 4, 7) for a in range(20)], 2, rng)     # every point in known voxels: no row, counts only
    before = W.A.host()
    assert W.extend(int(W.append(known)[1])).tolist() == [0, 401, 50, 0]
    a, R = W.check(3, "known voxels")
    assert a["count"][0] == 523 and a["count"][:401].sum() == 513 + 400 + 50 and same_bytes(a["normals"], before["normals"])
    W.close()
    # a new voxel next to old rows whose normal flips from invalid to valid: k = min_nbrs - 1 -> min_nbrs (mapgrow_np.FLIP)
    xyz, offs, kw = gnp.FLIP
    W = Rig(ctx, 4, 64, 8, 32, 1.0, nkw=kw)
    W.append(xyz[:3]); W.append(xyz[3:4])
    W.rebuild(n=1)
    a, _ = W.check(1, "before the flip", searches=False)
    assert a["ninfo"][:4].tolist() == [-3, -2, -2, 0]
    assert W.extend(1).tolist() == [1, 4, 1, 0]
    a, _ = W.check(2, "after the flip", searches=False)
    assert a["ninfo"][:5].tolist() == [4, -2, -2, -2, 0] and a["normals"][0, 2] > 0.99
    W.close(); ctx.close()


def test_colliding_keys_rule_edges_and_bad_poses():
    rng = np.random.default_rng(3)
    ctx = _stream_context(0)
    cells = np.array(mnp.COLLIDING_CELLS, np.float64)
    W = Rig(ctx, 8, 256, 64, 32, 1.0, nkw=dict(radius=0.99, min_nbrs=3, max_ratio=1.0))
    W.append(cells[0::2] + 0.5); W.append(cells[1::2] + 0.3 + 0.4 * rng.random((16, 3)))
    W.rebuild(n=1)                                                   # the 32 colliding cells: half rebuilt, half extended
    assert W.extend(1).tolist() == [16, 32, 16, 0]
    a, R = W.check(2, "colliding cells")
    assert R == 32 and set(map(tuple, np.floor(a["xyz"][:32]).astype(int))) == set(mnp.COLLIDING_CELLS)
    W.close()
    L = float(1 << 20)
    edge = np.array([(np.nan, 1, 1), (L - 0.5, 0.5, 0.5), (-L + 0.5, 0.5, 0.5), (L + 0.5, 0.5, 0.5), (0.5, -L - 0.5, 0.5), (-0.0, -0.0, -0.0),
                     (0.0, 0.25, 0.0), (-1e-300, 0.5, 0.5), (2.5, np.inf, 0.5), (L - 1.5, 0.5, 0.5)])
    W = Rig(ctx, 8, 256, 64, 32, 1.0, nkw=dict(radius=0.99, min_nbrs=3, max_ratio=1.0))
    W.append([(5.5, 5.5, 5.5)]); W.append(edge); W.append([(6.5, 5.5, 5.5), (7.5, 5.5, 5.5)]); W.append([(8.5, 5.5, 5.5)]); W.append([(9.5, 5.5, 5.5)])
    W.rebuild(n=1)
    info = W.extend(1)                                               # a NaN and an Inf point, the range's first and last voxel, one past each, -0.0
    assert info.tolist() == [5, 6, 6, wnp.SKIPPED | wnp.RANGE], info
    a, _ = W.check(2, "rule edges")
    assert a["count"][1:6].tolist() == [1, 1, 2, 1, 1] and np.signbit(a["xyz"][3]).all()      # -0.0 and (0, 0.25, 0) share voxel (0, 0, 0)
    poses = W.map_host()[3].copy()
    poses[2, 5] = np.nan; poses[3, 3] = np.inf                       # a pose row with a NaN, one with an Inf: fused advances, nothing stored
    assert W.extend(2, poses).tolist() == [0, 6, 0, wnp.SKIPPED]
    W.check(3, "NaN pose", poses)
    assert W.extend(3, poses).tolist() == [0, 6, 0, wnp.SKIPPED]
    W.check(4, "Inf pose", poses)
    assert W.extend(4, poses).tolist() == [1, 7, 1, 0]
    W.check(5, "a good row behind them", poses)
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the capacity and the refusals
def test_overflow_in_the_middle_of_a_cloud_then_full():
    D = gnp.drive()
    ctx = _stream_context(0)
    W = Rig(ctx, len(D["sizes"]) + 2, 2048, 600, 300, D["cell"])
    for k, c in enumerate(D["clouds"]):
        W.append(c, D["m_inten"][D["m_offs"][k]:D["m_offs"][k + 1]], D["poses"][k], k)
    W.rebuild(n=0)
    full = None
    for r in range(D["n"]):
        info = W.extend(r)
        if full is not None:
            assert info.tolist() == [0, 300, 0, gnp.FULL] and W.mg.count() == (full, 300, gnp.FULL), (r, info)
            W.check(full, ("refused", r), searches=False)
            continue
        W.check(r + 1, ("drive at 300", r))
        if info[3] & wnp.OVERFLOW:
            full = r + 1
            assert info[1] == 300 and 0 < info[0] < info[2]          # rows below the capacity and voxels past it in one cloud
    assert full is not None and full < D["n"]
    W.close(); ctx.close()


def test_the_committed_drive_the_host_forms_and_two_runs():
    """mapgrow_np.drive at out_capacity 2048: every keyframe through the device forms on one rig and through the host forms on another -
    the same bytes; a rebuild in the middle (n = 3) and extends behind it"""
    D = gnp.drive()
    ctx = _stream_context(0)
    rigs = [Rig(ctx, len(D["sizes"]) + 2, 2048, 600, 2048, D["cell"], model=(i == 0)) for i in range(2)]
    for W in rigs:
        for k, c in enumerate(D["clouds"]):
            W.append(c, D["m_inten"][D["m_offs"][k]:D["m_offs"][k + 1]], D["poses"][k], k)
        W.rebuild(n=0)
    W, H = rigs
    hn, hi = np.zeros((2048, 3)), np.zeros(2048, np.int32)
    for r in range(D["n"]):
        info = W.extend(r)
        a, R = W.check(r + 1, ("drive", r))
        hinfo = H.mg.extend(r, D["poses"] if r % 2 else None)        # the host forms: the poses uploaded or the map's own
        H.mg.normals(W.nkw["radius"], W.nkw["min_nbrs"], W.nkw["max_ratio"], hn, hi)
        assert hinfo.tolist() == info.tolist(), r
        h = H.A.host()
        for name in list(WORLD) + ["state"]:
            assert same_bytes(h[name], a[name]), ("host form / second run", r, name)
        assert hi.tolist() == a["ninfo"].tolist() and same_bytes(hn, a["normals"]), ("host normals", r)
        assert H.mg.count() == W.mg.count()
    assert (a["ninfo"] > 0).any()
    W.rebuild(n=3)
    for r in range(3, 6):
        W.extend(r)
        W.check(r + 1, ("behind a rebuild at 3", r))
    for W in rigs:
        W.close()
    ctx.close()


def test_refusals_change_nothing():
    D = gnp.drive()
    ctx = _stream_context(0)
    W = Rig(ctx, len(D["sizes"]) + 2, 2048, 600, 2048, D["cell"])
    for k, c in enumerate(D["clouds"][:5]):
        W.append(c, None, D["poses"][k], k)
    W.rebuild(n=3)
    a0, R = W.check(3, "rebuilt at 3")

    def unchanged(what, state=None):
        a = W.A.host()
        for name in a:
            if name != "state" or state is None:
                assert same_bytes(a[name], a0[name]), (what, name)
        assert W.A.ml.count() == W.B.ml.count() and W.mg.count()[:2] == (3, R), what

    for row, want in ((-1, 0), (-9, 0), (2, gnp.ORDER), (4, gnp.ORDER), (5, gnp.ORDER), (1 << 30, gnp.ORDER)):       # off; repeated; skipped; r >= n; scribbled
        assert W.extend(row).tolist() == [0, R, 0, want], row
        unchanged(("row", row))
    W.A.wm.state[0] = R - 2                                            # a fuse without a sync shows as another count
    W.M.state[0] = R - 2
    assert W.extend(3).tolist() == [0, R - 2, 0, gnp.STALE]
    assert W.extend(2).tolist() == [0, R - 2, 0, gnp.STALE | gnp.ORDER]
    for scribble, seen in ((1 << 30, 2048), (-5, 0)):                  # a scribbled world.state[0] is clamped before anything is addressed
        W.A.wm.state[0] = scribble; W.M.state[0] = scribble
        assert W.extend(3).tolist() == [0, seen, 0, gnp.STALE], scribble
    W.A.wm.state[0] = R; W.M.state[0] = R
    unchanged("stale")
    W.A.wm.state[1] = wnp.OVERFLOW; W.M.state[1] = wnp.OVERFLOW
    assert W.extend(3).tolist() == [0, R, 0, gnp.FULL] and W.mg.count() == (3, R, gnp.FULL)
    W.A.wm.state[1] = 0; W.M.state[1] = 0
    unchanged("full")
    B_rows = W.B.wm.fuse_torch(None, I32(2), W.cell, 1, "first")      # a real fuse without a sync, on the grower's own world map
    W.A.wm.fuse_torch(None, I32(2), W.cell, 1, "first"); W.A.ml.index_torch()
    torch.cuda.synchronize()
    R2 = int(B_rows.cpu()[0])
    assert R2 < R and W.mg.extend(3).tolist() == [0, R2, 0, gnp.STALE]
    W.rebuild(n=3)                                                     # and the accepted call goes through after the rebuild
    assert W.extend(3)[3] == 0
    W.check(4, "accepted after the refusals")
    other = _stream_context(0)
    with pytest.raises(ValueError, match="share one context"):
        api.MapGrower(other, W.A.wm, W.A.ml)
    with pytest.raises(ValueError, match="created over this world map"):
        api.MapGrower(ctx, W.A.wm, W.B.ml)
    h = C.c_void_p()
    assert ctx.lib.pr_mapgrow_create(ctx.h, W.A.wm.h, W.B.ml.h, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert "another world buffer record" in ctx.lib.pr_last_error(ctx.h).decode()
    assert ctx.lib.pr_mapgrow_create(other.h, W.A.wm.h, W.A.ml.h, C.byref(h)) == _lib.PR_EINVAL
    assert "another context" in ctx.lib.pr_last_error(other.h).decode()
    b = (C.c_double * 8)()
    assert ctx.lib.pr_mapgrow_normals_dev(W.mg.h, 0.4999, 5, 0.1, b, b) == _lib.PR_EINVAL and "exceeds the cell" in ctx.lib.pr_last_error(ctx.h).decode()
    other.close()
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. one captured graph
def test_one_graph_of_append_seed_refine_extend_normals():
    """ONE captured graph of append -> seed -> refine (against the rows of the earlier keyframes) -> extend -> normals, replayed over a
    switched-off call and three keyframes, equals the eager calls on a second rig and the rebuild"""
    D = gnp.drive(sizes=(255, 257, 290))
    nkw, cap = gnp.NORMALS, 300
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        rigs = [Rig(ctx, 6, 2048, cap, 1024, D["cell"], max_src=cap, model=False) for _ in range(2)]
        chains, outs = [], []
        for W in rigs:
            W.rebuild()
            x, it, offs = torch.zeros((cap, 3), dtype=torch.float64, device="cuda"), torch.zeros(cap, dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
            fr, pose, id_ = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros((1, 12), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            emitted = torch.zeros(4, dtype=torch.int32, device="cuda")
            (ainfo, g1), (T0, g2), (ps, g3) = guarded((4,), torch.int32), guarded((1, 3, 4), torch.float64), guarded((1,), torch.int32)
            (T, g4), (stats, g5) = guarded((1, 3, 4), torch.float64), guarded((1, api.ICP_STATS.itemsize), torch.uint8)
            row = ainfo[1:2]                                           # word 1 of the append's info: the first row or -1

            def chain(W=W, x=x, it=it, offs=offs, fr=fr, pose=pose, id_=id_, emitted=emitted, ainfo=ainfo, T0=T0, ps=ps, T=T, stats=stats, row=row):
                W.km.append_torch(x, it, offs, fr, poses=pose, ids=id_, emitted=emitted, max_points=cap, info=ainfo)
                W.A.ml.seed_torch(W.km.poses, W.km.state, row, src=row, out=(T0, ps))
                W.A.pl.refine_torch(W.km.xyz, W.km.offs, ps, T0, W.A.nrm, W.A.ninfo, out=(T, stats), min_inliers=6, **KW)
                W.mg.extend_torch(row, info=W.info)
                W.mg.normals_torch(nkw["radius"], nkw["min_nbrs"], nkw["max_ratio"], W.A.nrm, W.A.ninfo)

            chains.append((chain, (x, it, offs, pose, id_, emitted)))
            outs.append(((ainfo, T0, ps, T, stats, W.info), (g1, g2, g3, g4, g5, W.ginfo)))
        for chain, _ in chains:                                        # eager once with the call switched off: nothing changes
            chain()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            chains[0][0]()
        for count in range(4):
            got = []
            for i, (chain, (x, it, offs, pose, id_, emitted)) in enumerate(chains):
                if count:
                    c = D["clouds"][count - 1]
                    x.zero_(); x[:len(c)] = dev(c); it[:len(c)] = dev(np.linspace(0, 1, len(c)), np.float32)
                    offs[1] = len(c); pose[0] = dev(D["poses"][count - 1]); id_[0] = count; emitted[0] = 1
                for t in outs[i][0]:
                    t.fill_(GUARD)
                g.replay() if i == 0 else chain()
                st.synchronize()
                for gd in outs[i][1]:
                    gd()
                rigs[i].A.intact()
                got.append([t.cpu().numpy().copy() for t in outs[i][0]] + list(rigs[i].A.host().values()))
            for a, b in zip(*got):
                assert a.tobytes() == b.tobytes(), count
            ainfo, _, ps, _, stats, info = got[0][:6]
            assert ainfo[1] == (count - 1 if count else -1) and ps[0] == ainfo[1]
            assert info[3] == 0 and info[2] == (len(D["clouds"][count - 1]) if count else 0)
            rigs[0].check(count, ("replayed", count))
            if count >= 2:                                             # the refinement ran against the rows of the earlier keyframes
                s = np.frombuffer(stats.tobytes(), api.ICP_STATS)[0]
                assert s["status"] != _lib.ICP_NO_PAIR and s["n_inl"] > 0, (count, s)
        del g
        for W in rigs:
            W.close()
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the drive
def test_the_drive_extended_keyframe_by_keyframe(seq07):
    """the seq07 drive of test_gpu_maploc.py: every keyframe appended, extended and its normals updated; the rebuild's bytes at three
    keyframes along the way and at the end"""
    ctx = _stream_context(0)
    CELL, OC = 3.0, 1 << 15
    W = Rig(ctx, KCAP, PCAP, MAXC, OC, CELL, nkw=dict(radius=0.99 * CELL, min_nbrs=4, max_ratio=0.3), max_src=1024, model=False)
    win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
    out = win.empty_out()
    ainfo = torch.zeros(4, dtype=torch.int32, device="cuda")
    einfo = torch.zeros(4, dtype=torch.int64, device="cuda")
    W.rebuild()
    nkw, stored = W.nkw, 0
    for p in range(len(seq07["pid"])):
        w, x, it, k, pid = pose_inputs(seq07, p)
        win.push_torch(dev(w), dev(x), dev(it, np.float32), I32(k), out=out)
        W.km.append_push(out, pose=dev(w), id=I32(pid), info=ainfo)
        W.mg.extend_torch(ainfo[1:2], info=einfo)                      # (a warm-up push appends nothing: row -1, the call is off)
        W.mg.normals_torch(nkw["radius"], nkw["min_nbrs"], nkw["max_ratio"], W.A.nrm, W.A.ninfo)
        n = int(ainfo.cpu()[2])
        stored += int(einfo.cpu()[0])
        if n in (1, 40, 80):
            W.check(n, ("drive", n))
    assert n == 110 and W.mg.count() == (110, stored, 0)
    a, R = W.check(110, "the end of the drive")
    assert R == stored and R > 500 and (a["ninfo"][:R] > 0).sum() > 100
    W.close(); ctx.close()
