"""The local submaps on the device (pr_submap, submap.hip) against the NumPy restatement (submap_np.py): out_xyz up to
out_offs[c], out_offs, out_rows and info byte for byte, at the smallest shapes at which each kernel can go wrong - clouds one below, at
and one above the wave (64) and the workgroup (256), two chunks of a row (513), more slots than a scan chunk would need only at
slot_capacity (70 here: the chunk of 256 is crossed by the 300-slot rig), every clamp and skip of the rule.  Guard words stand behind
every output and guard rows behind out_offs[c].  Nothing here provokes a fault: every out-of-range count, index or length is a clamp or
a skip in the rule, and the tests check the skip.

The corner scene: the device's pose against the planted one within 10 x the error the restatements (submap_np + icp_np) have against it,
measured here on the CPU (2.5e-3 rad, 1.9e-3 m -> 2.5e-2 rad, 1.9e-2 m); the decisions (rejected / accepted) as on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_np
import posegraph_np as pg
import submap_cases as cases
import submap_np as sn
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_online import KCAP, MAXC, PCAP, pose_inputs, seq07  # noqa: F401  (seq07: the drive's fixture)

pytestmark = pytest.mark.gpu

GUARD = -7
PAD = 5
NAMES = api.Submaps._fields
IMAX = 2 ** 31 - 1
SIZES9 = (65, 0, 513, 1, 63, 0, 64, 257, 513)                      # empty rows in the middle of a window; 513 = two chunks and a point


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Rig:
    """a map, a builder and guarded outputs: every output array PAD elements (xyz: rows) longer than stated, the excess and, before each
    run, the array itself filled with the guard pattern"""

    def __init__(self, S, w_max, P, M, K, map_points=4096, ctx=None):
        self.own = ctx is None
        self.ctx = ctx or _stream_context(0)
        self.S, self.w_max, self.P, self.M, self.K, self.map_points = S, w_max, P, M, K, map_points
        self.km = api.KeyframeMap(self.ctx, K, map_points, M)
        self.sb = api.SubmapBuilder(self.ctx, S, w_max, P, M, K)
        assert self.sb.scratch_bytes() > 0
        tdt = {np.int32: torch.int32, np.float64: torch.float64, np.int64: torch.int64}
        self.big = {n: torch.empty(int(np.prod(s)) + PAD * (3 if n == "xyz" else 1), dtype=tdt[dt], device="cuda") for n, (s, dt) in self.sb.shapes().items()}
        self.out = api.Submaps(*(self.big[n][:int(np.prod(s))].view(s) for n, (s, dt) in self.sb.shapes().items()))

    def load(self, xyz, offs, poses, n):
        """the map's buffers as the caller states them (offs may be scribbled); n is written as it is"""
        X = np.zeros((self.map_points, 3)); X[:len(xyz)] = xyz
        O = np.zeros(self.K + 1, np.int64); O[:len(offs)] = offs
        Pz = np.zeros((self.K, 12)); Pz[:len(poses)] = np.asarray(poses).reshape(-1, 12)
        self.X, self.O, self.Pz, self.n = X, O, Pz, int(n)
        self.km.xyz.copy_(dev(X)); self.km.offs.copy_(dev(O, np.int64)); self.km.poses.copy_(dev(Pz))
        self.km.state.copy_(torch.tensor([int(n), 0, 0, 0], dtype=torch.int32))

    def fill(self):
        for t in self.big.values():
            t.fill_(GUARD)

    def read(self, c):
        got = {}
        for name, (shape, dt) in self.sb.shapes().items():
            a = host(self.big[name])
            pad = PAD * (3 if name == "xyz" else 1)
            assert (a[-pad:] == GUARD).all(), (name, "a guard word was written")
            got[name] = a[:-pad].reshape(shape).copy()
        end = int(got["offs"][c])
        assert 0 <= end <= self.P and (got["xyz"][end:] == GUARD).all(), "a row at or behind out_offs[c] was written"
        got["xyz"] = got["xyz"][:end]
        return got

    def run(self, centers, avoid=None, **kw):
        self.fill()
        cen = dev(centers, np.int32)
        av = None if avoid is None else dev(avoid, np.int32)
        self.sb.build_torch(self.km, cen, av, out=self.out, **kw)
        self.ctx.sync()
        return self.read(len(centers))

    def want(self, centers, avoid=None, *, w, past_only=False, avoid_gap=0, max_pts=None):
        return sn.build(self.X, self.O, self.Pz, self.n, centers, avoid, slot_capacity=self.S, point_capacity=self.P, max_cloud_points=self.M,
                        keyframe_capacity=self.K, w=w, past_only=past_only, avoid_gap=avoid_gap, max_pts=min(self.P, IMAX) if max_pts is None else max_pts)

    def check(self, what, centers, avoid=None, **kw):
        got, want = self.run(centers, avoid, **kw), self.want(centers, avoid, **kw)
        for name in NAMES:
            assert same_bytes(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:4], got["info"], want["info"], got["rows"][:8])
        return got

    def close(self):
        self.sb.close(); self.km.close()
        if self.own:
            self.ctx.close()


def centre_list(n, c, seed):
    """c centres over -1 .. n with n - 1, n, the largest i32 and -1 among them"""
    rng = np.random.default_rng(seed)
    cen = rng.integers(-1, n + 1, c).astype(np.int64)
    for k, v in enumerate((n - 1, n, IMAX, -1, 0)):
        if k < c:
            cen[(3 * k + 1) % c] = v
    return cen


# ------------------------------------------------------------------------------------------------ 1. counts, cloud sizes, slots, windows
@pytest.mark.parametrize("n", [0, 1, 2, 3, 9])
def test_map_counts_cloud_sizes_slot_counts_and_windows(n):
    """maps of 0, 1, 2, 3, 9 keyframes with clouds of 0, 1, 63, 64, 65, 257, 513 points; c in 0, 1, 3, 65, slot_capacity; w in 0, 1, 2,
    w_max: windows cut at both ends of the map, empty rows inside them"""
    S, w_max = 70, 4
    rig = Rig(S, w_max, 110000, 513, 9)
    xyz, offs, poses = cases.random_map(SIZES9[:n], seed=n)
    rig.load(xyz, offs, poses, n)
    points = 0
    for c in (0, 1, 3, 65, S):
        for w in (0, 1, 2, w_max):
            cen = centre_list(n, c, seed=100 * c + w)
            avoid = None if (c + w) % 2 else np.roll(cen, 1) + 1
            got = rig.check((n, c, w), cen, avoid, w=w, past_only=bool(w == 2 and c == 3), avoid_gap=1, max_pts=4000)
            assert (got["offs"][c:] == got["offs"][c]).all() and (got["rows"][c:] == 0).all()
            assert got["info"][3] & ~(sn.NO_CENTER | sn.TRUNCATED) == 0
            points += int(got["offs"][c])
    assert points > 0 or n == 0
    rig.close()


def test_more_slots_than_a_scan_chunk_and_overflow_inside_a_later_chunk():
    """300 slots: the scan's chunk of 256 is crossed; point_capacity is reached inside the second chunk, where smaller slots still fit"""
    rig = Rig(300, 1, 9000, 513, 9)
    xyz, offs, poses = cases.random_map(SIZES9, seed=4)
    rig.load(xyz, offs, poses, 9)
    cen = np.array([(7 * k) % 9 for k in range(300)])
    got = rig.check("300 slots", cen, w=0)
    assert got["info"][0] == int((got["rows"][:, 0] > 0).sum()) and got["info"][3] == sn.OVERFLOW
    over = np.nonzero(got["rows"][:, 1] & sn.OVERFLOW)[0]
    assert over.min() >= 0 and (got["rows"][over.min():, 0] > 0).any()          # slots placed behind the first one that overflowed
    rig.check("300 slots, w = 1", cen, w=1, max_pts=600)
    rig.close()


# ------------------------------------------------------------------------------------------------ 2. the rule's corners
def nine(P=20000, shift=0.0, **kw):
    rig = Rig(8, 3, P, 513, 9, **kw)
    xyz, offs, poses = cases.random_map(SIZES9, seed=7, shift=shift)
    return rig, xyz, offs, poses


def test_centres_off_the_map_and_non_finite_poses():
    rig, xyz, offs, poses = nine()
    rig.load(xyz, offs, poses, 9)
    got = rig.check("centres", [-1, 8, 9, IMAX, -2 ** 31, 0], w=2)
    assert got["rows"].tolist()[:6] == [[0, 0], [3, 0], [0, 2], [0, 2], [0, 0], [3, 0]] and got["info"].tolist()[0] == 2
    bad = poses.copy()
    bad[4, 3] = np.nan                                               # row 4: a centre (slot 0), a neighbour (slots 1, 2)
    bad[6, 11] = np.inf
    rig.load(xyz, offs, bad, 9)
    got = rig.check("poses", [4, 3, 5, 6, 7], w=2)
    assert got["rows"].tolist()[:5] == [[0, 2], [4, 0], [3, 0], [0, 2], [3, 0]]
    rig.close()


def test_nan_and_negative_zero_points_and_a_utm_translation():
    rig, xyz, offs, poses = nine(shift=5.0e6)
    xyz = xyz.copy()
    xyz[offs[2] + 5, 0] = np.nan; xyz[offs[2] + 70] = -0.0           # in row 2: a centre of slot 0, a neighbour of slot 1
    xyz[offs[4] + 3, 2] = np.nan; xyz[offs[4] + 9, 1] = -0.0
    rig.load(xyz, offs, poses, 9)
    got = rig.check("utm", [2, 3, 4, 8], w=1)
    sl = got["xyz"][got["offs"][0]:got["offs"][1]]                   # slot 0 = rows 2, 1, 3: the centre's points as they are
    assert same_bytes(sl[:513], xyz[offs[2]:offs[3]]) and np.signbit(sl[70]).all() and np.isnan(sl[5, 0]) and not np.isnan(sl[5, 1:]).any()
    s1 = got["xyz"][got["offs"][1]:got["offs"][2]]                   # slot 1 = rows 3, 2, 4: row 2 through the arithmetic
    assert np.isnan(s1[1 + 5]).all() and np.isfinite(s1[1 + 70]).all() and np.abs(s1[1 + 70]).max() < 1e3
    rig.close()


def test_a_count_beyond_the_capacity_and_scribbled_offsets():
    rig, xyz, offs, poses = nine()
    for n in (9 + 50, IMAX, -3, -2 ** 31):
        rig.load(xyz, offs, poses, n)
        got = rig.check(("n", n), [0, 4, 8, 9], w=3)
        assert got["rows"].tolist()[:4] == ([[4, 0], [7, 0], [4, 0], [0, 2]] if n > 0 else [[0, 2]] * 4)
    scr = offs.copy()
    scr[3] = offs[2] - 5                                             # row 2: a negative length; row 3: 513 + 5 + 1 points > max_cloud_points
    rig.load(xyz, scr, poses, 9)
    got = rig.check("scribbled", [2, 3, 4, 1], w=2)
    assert got["rows"].tolist()[:4] == [[3, 0], [3, 0], [3, 0], [2, 0]]
    scr = offs.copy()
    scr[0] = -4; scr[5] = 2 ** 62; scr[6] = -2 ** 63                 # a negative start; lengths whose difference would wrap
    rig.load(xyz, scr, poses, 9)
    rig.check("scribbled 64-bit", [0, 1, 4, 5, 6, 7], w=2)
    rig.close()


def test_max_pts_met_exactly_and_exceeded_by_one_point():
    rig, xyz, offs, poses = nine()
    rig.load(xyz, offs, poses, 9)
    total = 63 + 1 + 0 + 513 + 64                                    # centre 4, w = 2: rows 4, 3, 5, 2, 6
    got = rig.check("exact", [4, 4, 4, 2], w=2, max_pts=total)
    assert got["rows"].tolist()[0] == [5, 0]
    got = rig.check("one short", [4, 4, 4, 2], w=2, max_pts=total - 1)
    assert got["rows"].tolist()[0] == [4, sn.TRUNCATED] and got["offs"][1] == total - 64
    got = rig.check("the centre itself", [2, 4], w=2, max_pts=512)
    assert got["rows"].tolist()[:2] == [[0, sn.TRUNCATED], [3, sn.TRUNCATED]]
    rig.close()


def test_point_capacity_reached_inside_slot_1_of_3():
    rig, xyz, offs, poses = nine(P=500)
    rig.load(xyz, offs, poses, 9)
    got = rig.check("overflow", [0, 2, 4], w=1, max_pts=600)         # 65, then 514 passes 500, then 64 goes behind slot 0
    assert got["offs"].tolist()[:4] == [0, 65, 65, 129] and got["rows"].tolist()[:3] == [[2, 0], [0, sn.OVERFLOW], [3, 0]]
    assert got["info"].tolist() == [2, 129, 0, sn.OVERFLOW]
    rig.close()


def test_the_avoid_band():
    rig, xyz, offs, poses = nine()
    rig.load(xyz, offs, poses, 9)
    cen = [4, 4, 4, 4, 4, 4]
    rig.check("NULL", cen, None, w=3, avoid_gap=2)
    got = rig.check("inside, equal, far, extremes", cen, [5, 4, 100, IMAX, -2 ** 31, 2], w=3, avoid_gap=1)
    assert got["rows"][:6, 0].tolist() == [5, 5, 7, 7, 7, 4]        # the centre is exempt: avoid == centre drops rows 3 and 5 only
    got = rig.check("gap 0", cen, [5, 4, 100, IMAX, -2 ** 31, 2], w=3, avoid_gap=0)
    assert got["rows"][:6, 0].tolist() == [6, 7, 7, 7, 7, 6]
    got = rig.check("the largest gap", cen, [5, 4, 100, IMAX, -2 ** 31, 2], w=3, avoid_gap=IMAX)
    assert got["rows"][:6, 0].tolist() == [1, 1, 1, 1, 7, 1]        # |r + 2^31| exceeds the largest i32: nothing wraps
    rig.close()


# ------------------------------------------------------------------------------------------------ 3. refusals with a handle
def test_refusals_with_a_handle_run_nothing():
    rig, xyz, offs, poses = nine()
    rig.load(xyz, offs, poses, 9)
    rig.fill()
    lib, sb, km = rig.ctx.lib, rig.sb, rig.km
    rec = _lib.MapBuffers(*(C.c_void_p(getattr(km, nm).data_ptr()) for nm in km.NAMES))
    cen = dev([1, 2], np.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    o = rig.out
    err = lambda: lib.pr_last_error(rig.ctx.h).decode()

    def call(c=2, prm=None, rec_=rec, **null):
        a = dict(poses=p(km.poses), n=p(km.state), cen=p(cen), xyz=p(o.xyz), offs=p(o.offs), rows=p(o.rows), info=p(o.info))
        a.update({k: None for k in null})
        prm = prm or _lib.SubmapParams(1, 0, 0, 100)
        assert lib.pr_submap_build_dev(sb.h, C.byref(rec_) if rec_ is not None else None, a["poses"], a["n"], a["cen"], None, c, C.byref(prm), a["xyz"],
                                       a["offs"], a["rows"], a["info"]) == _lib.PR_EINVAL
        return err()
    assert "c=9 outside 0 .. slot_capacity=8" in call(c=9) and "c=-1" in call(c=-1)
    assert "half_window=4 outside 0 .. w_max=3" in call(prm=_lib.SubmapParams(4, 0, 0, 100))
    assert "max_pts=0" in call(prm=_lib.SubmapParams(1, 0, 0, 0)) and "avoid_gap=-2" in call(prm=_lib.SubmapParams(1, 0, -2, 10))
    for name in ("poses", "n", "cen", "xyz", "offs", "rows", "info"):
        assert "a required pointer is NULL" in call(**{name: True}), name
    assert "map record" in call(rec_=None)
    assert "map record" in call(rec_=_lib.MapBuffers(None, *(C.c_void_p(getattr(km, nm).data_ptr()) for nm in km.NAMES[1:])))
    with pytest.raises(ValueError, match="share one context"):
        other = _stream_context(0)
        try:
            sb.build_torch(api.KeyframeMap(other, 9, 64, 16), cen, w=1)
        finally:
            other.close()
    rig.ctx.sync()
    for t in rig.big.values():
        assert (host(t) == GUARD).all()                              # nothing ran
    rig.close()


# ------------------------------------------------------------------------------------------------ 4. forms of the call
def test_host_form_two_runs_and_one_capture_for_every_count():
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        rig = Rig(8, 3, 20000, 513, 9, ctx=ctx)
        xyz, offs, poses = cases.random_map(SIZES9, seed=7)
        cen = torch.zeros(6, dtype=torch.int32, device="cuda")
        av = torch.zeros(6, dtype=torch.int32, device="cuda")
        kw = dict(w=2, avoid_gap=1, max_pts=900)
        rig.load(xyz[:0], offs[:1], poses[:0], 0)
        rig.fill()
        rig.sb.build_torch(rig.km, cen, av, out=rig.out, **kw)       # one eager call, then the capture of the same call at n = 0
        st.synchronize()
        assert rig.read(6)["info"].tolist() == [0, 0, 0, sn.NO_CENTER]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            rig.sb.build_torch(rig.km, cen, av, out=rig.out, **kw)
        for n, centres, avoid in ((3, [0, 1, 2, 3, -1, 2], [2, 2, 0, 0, 0, 9]), (9, [8, 4, 0, 2, 6, 9], [0, 5, 1, 2, 3, 4]), (5, [4, 4, 1, -1, 5, 3], [3, 1, 1, 1, 1, 1])):
            rig.load(xyz[:offs[n]], offs[:n + 1], poses[:n], n)
            cen.copy_(torch.tensor(centres, dtype=torch.int32)); av.copy_(torch.tensor(avoid, dtype=torch.int32))
            rig.fill()
            graph.replay()
            st.synchronize()
            replay = rig.read(6)
            eager = rig.check(("eager", n), centres, avoid, **kw)
            again = rig.run(centres, avoid, **kw)
            hostf = rig.sb.build(rig.km, centres, avoid, **kw)
            for name in NAMES:
                assert same_bytes(replay[name], eager[name]) and same_bytes(eager[name], again[name]), (n, name)
                assert same_bytes(np.asarray(getattr(hostf, name)), eager[name]), (n, name, "host form")
            assert eager["info"][0] > 0 and eager["info"][1] > 0
        hostf = rig.sb.build(rig.km, [], None, **kw)                  # c = 0: offs and info are still written
        assert not hostf.offs.any() and hostf.info.tolist() == [0, 0, 0, 0] and hostf.xyz.shape == (0, 3)
        del graph
        rig.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the plug-in check and the corner scene
@pytest.fixture(scope="module")
def corner():
    """the scene and, once, what the restatements make of it"""
    sc, K = cases.corner_scene(), cases.CORNER
    res = {}
    for w in (0, K["w"]):
        q, db = cases.corner_sets(sc, w)
        res[w] = icp_np.icp(q, db, sc["T0"], **K["icp"])
    return sc, res


class CornerRig:
    def __init__(self, sc):
        K = cases.CORNER
        self.ctx = _stream_context(0)
        self.rows, self.M = K["rows"], K["per_keyframe"]
        self.km = api.KeyframeMap(self.ctx, self.rows, self.rows * self.M, self.M)
        self.km.xyz.copy_(dev(sc["xyz"])); self.km.offs.copy_(dev(sc["offs"], np.int64)); self.km.poses.copy_(dev(sc["poses"]))
        self.km.state.copy_(torch.tensor([self.rows, 0, 0, 0], dtype=torch.int32))
        self.sb = api.SubmapBuilder(self.ctx, 4, 3, 4 * 7 * self.M, self.M, self.rows)

    def close(self):
        self.sb.close(); self.km.close(); self.ctx.close()


def test_w0_submaps_plug_into_icp_with_the_bytes_of_the_maps_own_clouds(corner):
    sc, _ = corner
    rig = CornerRig(sc)
    P = sc["poses"].reshape(-1, 3, 4)
    I, Q = np.array([3, 2, 4, 5], np.int32), np.array([13, 12, 14, 16], np.int32)
    T0 = dev(np.stack([pg.mul(P[i], pg.inv(P[q])) for i, q in zip(I, Q)]))
    di, dq = dev(I, np.int32), dev(Q, np.int32)
    kw = dict(max_iter=8, max_corr=0.6, min_inliers=3, ctx=rig.ctx)
    own = api.icp_refine_torch(rig.km.xyz, rig.km.offs, rig.km.xyz, rig.km.offs, dq, di, T0, rig.M, rig.M, **kw)
    db, q, ps, pd = rig.sb.pair_torch(rig.km, di, dq, w=0)
    sub = api.icp_refine_torch(q.xyz, q.offs, db.xyz, db.offs, ps, pd, T0, rig.M, rig.M, **kw)
    rig.ctx.sync()
    assert host(ps).tolist() == host(pd).tolist() == [0, 1, 2, 3]
    assert same_bytes(host(db.xyz)[:4 * rig.M], np.concatenate([sc["xyz"][i * rig.M:(i + 1) * rig.M] for i in I]))
    assert same_bytes(host(own[0]), host(sub[0])) and same_bytes(host(own[1]), host(sub[1]))
    stats = host(sub[1]).view(api.ICP_STATS).reshape(-1)
    assert (stats["iters"] > 0).any()                                # the refinement did run
    rig.close()


def test_corner_scene_single_clouds_are_rejected_and_w3_submaps_recover_the_pose(corner):
    sc, res = corner
    K = cases.CORNER
    want_single, want_sub = res[0], res[K["w"]]
    ref_err = cases.pose_error(want_sub["T"], sc["T_true"])          # the restatements' own error against the planted pose
    rig = CornerRig(sc)
    i, q = sc["pair"]
    di, dq, T0 = dev([i], np.int32), dev([q], np.int32), dev(sc["T0"][None])
    kw = dict(ctx=rig.ctx, **K["icp"])
    single = api.icp_refine_torch(rig.km.xyz, rig.km.offs, rig.km.xyz, rig.km.offs, dq, di, T0, rig.M, rig.M, **kw)
    db, qs, ps, pd = rig.sb.pair_torch(rig.km, di, dq, w=K["w"], avoid_gap=K["w"])
    max_pts = 7 * rig.M
    sub = api.icp_refine_torch(qs.xyz, qs.offs, db.xyz, db.offs, ps, pd, T0, max_pts, max_pts, **kw)
    rig.ctx.sync()
    assert host(db.rows)[0].tolist() == [7, 0] and host(qs.rows)[0].tolist() == [4, 0]
    s0 = host(single[1]).view(api.ICP_STATS).reshape(-1)[0]
    s3 = host(sub[1]).view(api.ICP_STATS).reshape(-1)[0]
    got_err = cases.pose_error(host(sub[0])[0], sc["T_true"])
    print(f"   corner scene: restatement error {ref_err}, device error {got_err}, bound 10 x; single n_inl {s0['n_inl']} status {s0['status']}, "
          f"submaps n_inl {s3['n_inl']} fitness {s3['fitness']:.3f} rmse {s3['rmse']:.4f}")
    assert not api.icp_accept(np.array([s0]), K["min_fitness"], K["max_rmse"])[0] and s0["status"] == _lib.ICP_TOO_FEW == want_single["status"]
    assert api.icp_accept(np.array([s3]), K["min_fitness"], K["max_rmse"])[0] and s3["n_inl"] == want_sub["n_inl"]
    assert got_err[0] <= 10 * ref_err[0] and got_err[1] <= 10 * ref_err[1]
    rig.close()


# ------------------------------------------------------------------------------------------------ 6. the drive
def test_the_drive_search_submaps_refine_as_one_graph(seq07):
    """the seq07 map (110 keyframes behind 30 warm-up pushes): search -> pair_torch -> refine captured once and replayed for two query
    ranges equals the eager bytes"""
    P, Q, W, MAXP = len(seq07["pid"]), 4, 1, 3 * MAXC
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((60, 3), dtype=torch.float64, device="cuda")
        it = torch.zeros(60, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        kid = torch.zeros(1, dtype=torch.int32, device="cuda"); minfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
        km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
        out = win.empty_out()
        for i in range(P):
            w, hx, hit, k, pid = pose_inputs(seq07, i)
            pose.copy_(torch.from_numpy(w.copy())); x.copy_(torch.from_numpy(hx)); it.copy_(torch.from_numpy(hit)); n.fill_(k); kid.fill_(pid)
            win.push_torch(pose, x, it, n, out=out)
            km.append_push(out, pose=pose, id=kid, info=minfo)
        st.synchronize()
        assert host(km.state).tolist() == [110, 0, 0, 0]
        ps = api.ProximitySearch(ctx, KCAP, Q, 1)
        sb = api.SubmapBuilder(ctx, Q, W, Q * MAXP, MAXC)              # no keyframe_capacity: the first (eager) call takes the map's
        qr = torch.tensor([60, Q], dtype=torch.int32, device="cuda")
        skw = dict(radius=50.0, min_gap=5, k=1)
        keep = dict(cand=None, pair=None, ref=None)

        def chain():
            keep["cand"] = ps.search_map(km, qr, out=keep["cand"], **skw)
            cand = keep["cand"]
            db, q, src, dst = sb.pair_torch(km, cand.pair_dst, cand.pair_src, w=W, avoid_gap=W, max_pts=MAXP, out=keep["pair"])
            keep["pair"] = (db, q)
            keep["ref"] = api.icp_refine_torch(q.xyz, q.offs, db.xyz, db.offs, src, dst, cand.T0, MAXP, MAXP, max_iter=4, max_corr=1.0, ctx=ctx,
                                               out=keep["ref"])

        def read():
            st.synchronize()
            db, q = keep["pair"]
            got = dict(T=host(keep["ref"][0]).copy(), stats=host(keep["ref"][1]).copy(), src=host(keep["cand"].pair_src).copy())
            for tag, s in (("db", db), ("q", q)):
                o = host(s.offs)
                got.update({tag + "_offs": o.copy(), tag + "_rows": host(s.rows).copy(), tag + "_info": host(s.info).copy(),
                            tag + "_xyz": host(s.xyz)[:int(o[Q])].copy()})
            return got

        chain()                                                      # eager first: the ICP scratch grows here, not in the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            chain()
        offs = host(km.offs)
        for q0 in (60, 106):
            qr.copy_(torch.tensor([q0, Q], dtype=torch.int32))
            graph.replay()
            replay = read()
            chain()
            eager = read()
            for name in eager:
                assert same_bytes(replay[name], eager[name]), (q0, name)
            assert eager["src"].tolist() == list(range(q0, q0 + Q)) and eager["db_info"][0] == Q and eager["q_info"][0] == Q
            assert eager["db_rows"][:, 0].tolist() == [3] * Q and eager["q_rows"][:, 0].tolist() == [2] * Q
            own = [int(offs[r + 1] - offs[r]) for r in range(q0, q0 + Q)]
            assert (np.diff(eager["q_offs"]) > np.array(own)).all()   # every query submap holds more than its centre's cloud
            stats = eager["stats"].view(api.ICP_STATS).reshape(-1)
            assert (stats["n_inl"] > 0).all()
        del graph
        sb.close(); ps.close(); km.close(); win.close(); ctx.close()
