"""The pose-proximity candidate search and the batch add of the closure log on the device (pr_proximity, proximity.hip; pr_posegraphb_add,
posegraph.hip) against the NumPy restatement (proximity_np.py): idx, d2, T0, pair_src, pair_dst, known and info byte for
byte, at the smallest shapes at which each part can go wrong - one below, at and one above the kernel's tile rows (16) and slab columns
(256), one run and merged runs, every clamp of the rule.  Guard words stand behind every output.  Nothing here provokes a fault: every
out-of-range count or index is a clamp or a skip in the rule, and the tests check the skip.

The chain scene: T of the device ICP against icp_np by test_gpu_icp.py's rule (status, iters, n_inl, fitness equal; rmse, R, t within
1e-10 = 100 x the 1e-12 the order of the restatement's own sums moves them); the relaxed poses within test_gpu_posegraph.py's bound()."""
import numpy as np
import pytest
import torch

import gate_np
import posegraph_np as pg
import proximity_np as px
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context

pytestmark = pytest.mark.gpu

GUARD = -7
PAD = 5
NAMES = api.Proximity._fields
ROWS, COLS = 16, 256
EPS = 2.0 ** -52
ICP_TOL = 1e-10


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def drive():
    """520 keyframes on two laps of a circle of 6 m under odometry noise, made once: every count below takes its first n rows"""
    return px.two_lap_circle(520, seed=2, radius=6.0, rot=0.004, trans=0.02)


class Rig:
    """a handle and guarded outputs: every array PAD elements longer than stated - rows beyond query_capacity -, the excess and, before
    each run, the array itself filled with the guard pattern"""

    def __init__(self, cap, Q, k_max, ctx=None):
        self.own = ctx is None
        self.ctx = ctx or _stream_context(0)
        self.cap, self.Q = cap, Q
        self.ps = api.ProximitySearch(self.ctx, cap, Q, k_max)
        assert self.ps.tile() == (ROWS, COLS) and self.ps.scratch_bytes() > 0
        self.poses = torch.zeros((cap, 12), dtype=torch.float64, device="cuda")
        self.nd = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
        self.qr = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.big = {}

    def outs(self, k):
        if k not in self.big:
            tdt = {np.int32: torch.int32, np.float64: torch.float64, np.uint8: torch.uint8}
            self.big[k] = {n: torch.empty(int(np.prod(s)) + PAD, dtype=tdt[dt], device="cuda") for n, (s, dt) in self.ps.shapes(k).items()}
        big = self.big[k]
        return big, api.Proximity(*(big[n][:big[n].numel() - PAD] for n in NAMES))

    def load(self, P, n, qrange):
        buf = np.zeros((self.cap, 12))
        P = np.asarray(P, np.float64).reshape(-1, 12)[:self.cap]
        buf[:len(P)] = P
        self.P_np = buf
        self.poses.copy_(dev(buf))
        self.nd[0] = int(n)
        self.qr.copy_(torch.tensor(list(qrange), dtype=torch.int32))
        self.n, self.qrange = int(n), tuple(int(x) for x in qrange)

    def run(self, log=None, **kw):
        big, out = self.outs(kw.get("k", 1))
        for t in big.values():
            t.fill_(GUARD % 256 if t.dtype == torch.uint8 else GUARD)
        self.ps.search_torch(self.poses, self.nd, self.qr, log=log, out=out, **kw)
        self.ctx.sync()
        return self.read(kw.get("k", 1))

    def read(self, k):
        got = {}
        for name, (shape, dt) in self.ps.shapes(k).items():
            a = host(self.big[k][name])
            assert (a[-PAD:] == (GUARD % 256 if dt == np.uint8 else GUARD)).all(), (name, "a guard word was written")
            got[name] = a[:-PAD].reshape(shape).copy()
        return got

    def want(self, log=None, log_edge_capacity=0, **kw):
        return px.search(self.P_np, self.n, self.qrange, self.cap, self.Q, log=log, log_edge_capacity=log_edge_capacity, **kw)

    def check(self, what, log=None, log_np=None, log_cap=0, **kw):
        got, want = self.run(log=log, **kw), self.want(log=log_np, log_edge_capacity=log_cap, **kw)
        for name in NAMES:
            assert same_bytes(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:4], got["info"], want["info"])
        return got

    def close(self):
        self.ps.close()
        if self.own:
            self.ctx.close()


KW = dict(radius=2.5, growth=0.02, radius_max=5.0, min_gap=5, stride=3, k=4)


# ------------------------------------------------------------------------------------------------ 1. counts, capacities, tiles, runs
@pytest.mark.parametrize("cap,Q", [(256, 256), (257, 257), (600, 600), (2048, 2048), (2048, 17), (15, 15), (16, 16), (17, 17)])
def test_counts_and_capacities(drive, cap, Q):
    """C = 1, 2, 3, 8 blocks of the prefix; one run (cap <= 256, or 128 tiles and more) and 2, 3, 8 merged runs; rows and columns one
    below, at and one above the tile"""
    rig = Rig(cap, Q, 4)
    filled = 0
    for n in (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513):
        if n > cap:
            continue
        q0 = max(0, n - Q)                                          # the last Q rows where the handle holds fewer than n
        rig.load(drive[:n], n, (q0, min(n, Q)))
        got = rig.check((cap, Q, n), **KW)
        assert got["info"][0] == min(n, Q) and got["info"][3] == 0
        filled += int(got["info"][1])
    assert filled > 0 or cap < 6
    rig.close()


# ------------------------------------------------------------------------------------------------ 2. query ranges, scribbled counts
def test_query_ranges_and_scribbled_counts(drive):
    rig = Rig(300, 40, 2)
    P = drive[:300].copy()
    P[33, 7] = np.nan
    kw = dict(radius=2.5, min_gap=5, k=2)
    for n, qr, flag, rows in ((300, (0, 40), 0, 39), ((300), (260, 40), 0, 40), (300, (280, 40), 1, 20), (300, (-10, 40), 1, 30), (300, (0, 0), 0, 0),
                              (300, (20, 99), 1, 39), (300, (20, -4), 1, 0), (300, (2 ** 31 - 8, 40), 1, 0), (300, (-2 ** 31, 40), 1, 0),
                              (-5, (0, 40), 1, 0), (10 ** 9, (270, 40), 1, 30), (120, (100, 40), 1, 20)):
        rig.load(P, n, qr)
        got = rig.check((n, qr), **kw)
        assert got["info"][3] == flag and got["info"][0] == rows, (n, qr, got["info"])
    rig.close()


# ------------------------------------------------------------------------------------------------ 3. k, stride, min_gap
@pytest.mark.parametrize("k,stride,min_gap", [(1, 1, 5), (4, 1, 1), (32, 1, 5), (32, 8, 5), (4, 3, 5), (4, 8, 299), (4, 1000, 5), (2, 3, 300),
                                              (2, 3, 2 ** 31 - 1), (32, 2 ** 31 - 1, 1)])
def test_k_stride_and_min_gap(drive, k, stride, min_gap):
    """stride 3 and 8 against slabs of 256 and runs cut at bucket borders: buckets straddle slab borders, never run borders; k = 32 is more
    than the candidates of most rows; min_gap = n - 1 leaves one pair, min_gap >= n none"""
    rig = Rig(600, 300, 32)
    rig.load(drive[:300], 300, (0, 300))
    got = rig.check((k, stride, min_gap), radius=2.5, growth=0.05, radius_max=6.0, min_gap=min_gap, stride=stride, k=k)
    if min_gap >= 300:
        assert got["info"][1] == 0
    elif min_gap == 5:
        assert got["info"][1] > (150 if k == 1 or stride >= 1000 else 300)      # one bucket a row: at most one slot a row
        if stride == 1 and k == 32:
            assert (got["idx"][:, -1] == -1).any() and (got["idx"][:, 8] >= 0).any()
    rig.close()


# ------------------------------------------------------------------------------------------------ 4. an integer lattice: exact d2 and rad^2
LATTICE = [(3, 4, 0), (4, 3, 0), (0, 0, 5), (2, 2, 4), (4, 2, 2), (1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]


def test_integer_lattice_radius_ties_and_standstill():
    rig = Rig(16, 16, 16)
    P = px.lattice_poses(LATTICE, yaw=np.arange(len(LATTICE)))
    assert (np.signbit(P) & (P == 0.0)).any()                        # the rows carry -0.0
    rig.load(P, 12, (0, 12))
    at = rig.check("at the radius", radius=5.0, min_gap=1, k=16)
    assert at["idx"][11].tolist()[:9] == [7, 8, 9, 10, 5, 6, 3, 4, -1]                          # d2 = 25 at radius 5 is out; ties: the lower row
    assert at["d2"][11].tolist()[:8] == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 24.0, 24.0]
    inside = rig.check("one ulp inside", radius=float(np.nextafter(5.0, 6.0)), min_gap=1, k=16)
    assert inside["idx"][11].tolist()[:12] == [7, 8, 9, 10, 5, 6, 3, 4, 0, 1, 2, -1]
    two = rig.check("buckets of two", radius=5.0, min_gap=1, stride=2, k=16)
    assert two["idx"][11].tolist()[:6] == [7, 8, 10, 5, 3, -1]       # buckets {6, 7}, {8, 9}, {10}, {4, 5}, {2, 3}: ties inside and across
    rig.check("standstill steps", radius=5.0, growth=1.0, radius_max=7.0, min_gap=1, stride=2, k=3)
    # a line: row a at (a, 0, 0), then the query back at the origin: s[q] - s[i] = 16 - i, rad = 1 + (16 - i) / 4 = 5 - i / 4, all exact
    line = [(a, 0, 0) for a in range(9)] + [(0, 0, 0)]
    rig.load(px.lattice_poses(line), 10, (9, 1))
    for rmax, want in ((4.0, [0, 1, 2, 3]), (4.5, [0, 1, 2, 3]), (4.25, [0, 1, 2, 3]), (3.0, [0, 1, 2])):
        got = rig.check(("radius_max", rmax), radius=1.0, growth=0.25, radius_max=rmax, min_gap=1, k=16)
        assert got["idx"][0].tolist()[:len(want) + 1] == want + [-1], (rmax, got["idx"][0])   # i = 4: rad meets 4.0, d2 = 16 is not below 16
    rig.close()


# ------------------------------------------------------------------------------------------------ 5. non-finite and extreme rows
def test_non_finite_rows_a_utm_route_and_negative_zero(drive):
    rig = Rig(600, 300, 4)
    P = drive[:300].copy()
    P[40, 3] = np.nan                                                # a DB row, in the middle of the prefix
    P[150, 0] = np.inf
    P[299, 11] = -np.inf                                             # the newest query row
    P[200] = np.nan
    rig.load(P, 300, (0, 300))
    got = rig.check("non-finite", **KW)
    assert got["info"][0] == 296 and not np.isin(got["idx"], (40, 150, 200, 299)).any() and (got["idx"][[40, 150, 200, 299]] == -1).all()
    U = drive[:300].reshape(-1, 3, 4).copy()                         # the same route at a UTM northing: c' = c + o, t' = t - R o
    U[:, :, 3] -= U[:, :, :3] @ np.array([4.0e5, 5.0e6, 30.0])
    rig.load(U.reshape(-1, 12), 300, (0, 300))
    far = rig.check("utm", **KW)
    assert far["info"][1] > 100
    Z = np.zeros((300, 12))                                          # all-zero rows: every centre (-0.0, -0.0, -0.0), every step 0
    Z[:, 0] = -0.0
    rig.load(Z, 300, (0, 300))
    rig.check("zeros", **KW)
    rig.close()


# ------------------------------------------------------------------------------------------------ 6. heading
def test_heading_with_a_pass_in_the_opposite_direction():
    out = [(a, 0, 0) for a in range(20)]
    back = [(19 - a, 1, 0) for a in range(20)]
    side = [(a, 2, 0) for a in range(10)]
    P = px.lattice_poses(out + back + side, yaw=[0] * 20 + [2] * 20 + [1] * 10)       # along +x, along -x, along +y
    rig = Rig(64, 64, 8)
    rig.load(P, 50, (0, 50))
    counts = []
    for cm in (-1.0, 0.0, 0.5, 1.0):
        got = rig.check(("cos_min", cm), radius=2.5, min_gap=2, k=8, cos_min=cm)
        counts.append(int(got["info"][1]))
    assert counts[0] > counts[1] > counts[2] == counts[3] > 0        # -1: all; 0: not the opposite pass; 0.5, 1: the same direction only
    rig.close()


# ------------------------------------------------------------------------------------------------ 7. the log
def guarded(ctx, cap, node_capacity=600):
    """a graph over buffers one row / four words longer than stated, the excess filled with a guard pattern"""
    big = dict(edge_ij=torch.zeros((cap + 1, 2), dtype=torch.int32, device="cuda"), edge_Z=torch.zeros((cap + 1, 12), dtype=torch.float64, device="cuda"),
               edge_w=torch.zeros((cap + 1, 2), dtype=torch.float64, device="cuda"), state=torch.zeros(8, dtype=torch.int32, device="cuda"))
    for n in ("edge_ij", "edge_Z", "edge_w"):
        big[n][cap:] = GUARD
    big["state"][4:] = GUARD
    g = api.PoseGraph(ctx, node_capacity, cap, buffers={n: (t[:4] if n == "state" else t[:cap]) for n, t in big.items()})

    def intact():
        assert all(bool((big[n][cap:] == GUARD).all()) for n in ("edge_ij", "edge_Z", "edge_w")) and bool((big["state"][4:] == GUARD).all())
    return g, intact, big


def test_known_pairs_of_the_log(drive):
    ctx = _stream_context(0)
    rig = Rig(600, 300, 4, ctx=ctx)
    EC = 70
    g, intact, big = guarded(ctx, EC)
    rig.load(drive[:300], 300, (0, 300))
    free = rig.check("no log", **KW)
    assert not free["known"].any() and free["info"][2] == 0
    empty = rig.check("empty log", log=g, log_np=(np.zeros((EC, 2), np.int32), np.zeros(4, np.int32)), log_cap=EC, known_window=2, **KW)
    assert same_bytes(empty["T0"], free["T0"])
    slots = np.flatnonzero(free["pair_src"] >= 0)
    e = np.full((EC, 2), -1, np.int32)
    pick = slots[:: max(1, len(slots) // 60)][:60]
    for a, o in enumerate(pick):
        i, q = int(free["pair_dst"][o]), int(free["pair_src"][o])
        e[a] = [(i, q), (q, i), (i + 2, q - 1), (-1, q), (i, -1)][a % 5]      # both orientations, near misses, negative indices
    g.edge_ij.copy_(dev(e, np.int32))
    for state0, window in ((60, 0), (60, 2), (25, 1), (10 ** 6, 0), (-4, 2), (EC, 2 ** 31 - 1)):
        g.state[0] = state0
        got = rig.check(("log", state0, window), log=g, log_np=(e, np.array([state0, 0, 0, 0])), log_cap=EC, known_window=window, **KW)
        assert same_bytes(got["idx"], free["idx"]) and same_bytes(got["d2"], free["d2"])
        if state0 == 60:
            assert got["info"][2] >= (24 if window == 0 else 36)
        if state0 < 0:
            assert got["info"][2] == 0
        if window == 2 ** 31 - 1:
            assert got["info"][2] == got["info"][1]                  # every filled slot is near some edge
    intact()
    rig.close(); g.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 8. forms of the call
def test_host_form_two_runs_and_one_capture_for_every_count(drive):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        rig = Rig(600, 64, 4, ctx=ctx)
        g, intact, _ = guarded(ctx, 8)
        e = np.array([[3, 40], [200, 10], [-1, 5], [7, 7], [0, 0], [0, 0], [0, 0], [0, 0]], np.int32)
        g.edge_ij.copy_(dev(e, np.int32))
        kw = dict(KW, known_window=3)
        rig.load(drive[:0], 0, (0, 0))
        rig.run(log=g, **kw)                                         # one eager call, then the capture of the same call at n = 0
        big, out = rig.outs(4)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            rig.ps.search_torch(rig.poses, rig.nd, rig.qr, log=g, out=out, **kw)
        for n, qr, edges in ((70, (6, 64), 1), (513, (449, 64), 2), (300, (250, 64), 4)):
            rig.load(drive[:n], n, qr)
            g.state[0] = edges
            for t in big.values():
                t.fill_(GUARD % 256 if t.dtype == torch.uint8 else GUARD)
            graph.replay()
            st.synchronize()
            replay = rig.read(4)
            log_np = (e, np.array([edges, 0, 0, 0]))
            eager = rig.check((n, qr), log=g, log_np=log_np, log_cap=8, **kw)
            again = rig.run(log=g, **kw)
            hostf = rig.ps.search(rig.poses, rig.nd, rig.qr, log=g, **kw)
            for name in NAMES:
                assert same_bytes(replay[name], eager[name]) and same_bytes(eager[name], again[name]), (n, name)
                assert same_bytes(np.asarray(getattr(hostf, name)), eager[name]), (n, name, "host form")
            assert eager["info"][1] > 0
        intact()
        del graph
        rig.close(); g.close(); ctx.close()


def test_host_form_without_known(drive):
    """pr_proximity_search with known = NULL (allowed without a closure log): every output that was passed equals, byte for byte, that of
    the call with all outputs, at the file's smallest rig"""
    import ctypes as C
    rig = Rig(15, 15, 4)
    rig.load(drive[:15], 15, (0, 15))
    full = rig.ps.search(rig.poses, rig.nd, rig.qr, **KW)
    assert full.info[1] > 0
    # ProximitySearch.search always allocates and passes every output, so known = NULL is reachable through the C entry point alone; the
    # params record is built by the class's own helper so that it is the one search() passed above
    k, prm, rec, ec = rig.ps._args("test", rig.poses, rig.nd, rig.qr, KW["radius"], KW["growth"], KW["radius_max"], -1.0, KW["min_gap"], KW["stride"],
                                   KW["k"], None, 0)
    got = {name: np.full(shape, GUARD % 256 if dt == np.uint8 else GUARD, dt) for name, (shape, dt) in rig.ps.shapes(k).items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    outs = [None if name == "known" else got[name].ctypes.data_as(C.c_void_p) for name in NAMES]
    rig.ctx.check(rig.ctx.lib.pr_proximity_search(rig.ps.h, p(rig.poses), p(rig.nd), p(rig.qr), C.byref(prm), None, ec, *outs))
    for name in NAMES:
        if name != "known":
            assert same_bytes(got[name], np.asarray(getattr(full, name))), name
    rig.close()


# ------------------------------------------------------------------------------------------------ 9. the batch add
def batch_inputs(c, seed):
    rng = np.random.default_rng(seed)
    i = rng.integers(-1, 50, c).astype(np.int32)
    j = rng.integers(-1, 50, c).astype(np.int32)
    T = rng.normal(size=(c, 12))
    T[rng.random(c) < 0.1, 5] = np.nan
    acc = (rng.random(c) < 0.8).astype(np.uint8)
    w = rng.uniform(0.0, 5.0, (c, 2))
    for bad in (np.nan, -1.0, np.inf):
        w[rng.random(c) < 0.05, rng.integers(0, 2)] = bad
    return i, j, T, acc, w


def assert_log(g, model, what):
    for n in api.PoseGraph.NAMES:
        assert same_bytes(host(getattr(g, n)), getattr(model, n)), (what, n)


@pytest.mark.parametrize("c,cap,with_w", [(1, 8, True), (5, 8, False), (256, 100, True), (257, 400, True), (1025, 500, False), (1025, 2000, True)])
def test_batch_add_equals_the_restatement_and_single_adds(c, cap, with_w):
    ctx = _stream_context(0)
    g, intact, big = guarded(ctx, cap)
    single, hostg = api.PoseGraph(ctx, 600, cap), api.PoseGraph(ctx, 600, cap)
    model = pg.PoseGraphModel(cap)
    i, j, T, acc, w = batch_inputs(c, c)
    wd = dev(w) if with_w else None
    info_big = torch.full((4 + PAD,), GUARD, dtype=torch.int32, device="cuda")
    seen_overflow = False
    for call, state0 in enumerate((0, None, 10 ** 6 if cap < 450 else -9)):    # empty, on top of the first call, a scribbled count
        if state0 is not None and call:
            for x in (g, single, hostg):
                x.state[0] = state0
            model.state[0] = state0
        info = g.add_batch_torch(dev(i, np.int32), dev(j, np.int32), dev(T), dev(acc, np.uint8), wd, 2.0, 3.0, info=info_big[:4])
        want = px.add_batch(model, i, j, T, acc, w if with_w else None, 2.0, 3.0)
        ctx.sync()
        assert host(info).tolist() == want.tolist() and bool((info_big[4:] == GUARD).all()), (call, host(info), want)
        assert_log(g, model, call)
        intact()
        assert hostg.add_batch(i, j, T, acc, w if with_w else None, 2.0, 3.0).tolist() == want.tolist()
        assert_log(hostg, model, ("host", call))
        wc = dev(w if with_w else np.tile([2.0, 3.0], (c, 1)))
        ii, jj, TT, aa = dev(i, np.int32), dev(j, np.int32), dev(T), dev(acc, np.uint8)
        for p in range(c):                                          # c calls of pr_posegraphw_add_dev with k = 1
            single.add_weighted_torch(ii[p:p + 1], TT[p:p + 1], aa[p:p + 1], jj[p:p + 1], wc[p:p + 1])
        ctx.sync()
        assert_log(single, model, ("single", call))
        seen_overflow |= bool(want[3])
    assert seen_overflow or not (cap <= 500 and c >= 256)           # the batches of 256 and more run across the small capacities
    assert not (seen_overflow and cap == 2000)
    for x in (g, single, hostg):
        x.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 10. the chain scene on the device
def test_chain_scene_search_verify_log_gate_relax():
    sc, run, c = px.chain_scene(), px.chain_run(), px.CHAIN
    n, k = c["n"], c["search"]["k"]
    res = run["search"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        pts = sum(len(x) for x in sc["clouds"])
        km = api.KeyframeMap(ctx, n, pts, 1024, max_append=n)
        offs = np.concatenate([[0], np.cumsum([len(x) for x in sc["clouds"]])]).astype(np.int64)
        km.append(np.concatenate(sc["clouds"]), np.zeros(pts, np.float32), offs, np.zeros((n, 16)), poses=sc["est"])
        ps = api.ProximitySearch(ctx, n, n, k)
        EC = 256
        log, dst = api.PoseGraph(ctx, n, EC, max_outer=6, max_inner=480), api.PoseGraph(ctx, n, EC, max_outer=6, max_inner=480)
        gate = api.ClosureGate(ctx, log, dst, **c["gate"])
        qr = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        cand = ps.search_map(km, qr, **c["search"])
        T, stats, accepted = ps.verify_map_torch(km, cand, 1024, min_fitness=c["min_fitness"], max_rmse=c["max_rmse"], **c["icp"])
        info = log.add_batch_torch(cand.pair_dst, cand.pair_src, T, accepted, None, *c["w"])
        keep, support, mp, ginfo = gate.run_map(km)
        relaxed, report = dst.relax_map(km, **c["relax"])
        ctx.sync()
        for name in NAMES:                                           # the search: the restatement's bytes
            assert same_bytes(host(getattr(cand, name)), res[name]), name
        slots = run["slots"]
        s = host(stats).view(api.ICP_STATS).reshape(-1)
        Td = host(T).reshape(-1, 12)
        off = np.setdiff1d(np.arange(n * k), slots)
        assert (s["status"][off] == _lib.ICP_NO_PAIR).all() and not host(accepted)[off].any()
        worst = 0.0
        for a, o in enumerate(slots):                                # the ICP: test_gpu_icp.py's rule
            assert (s["status"][o], s["iters"][o], s["n_inl"][o]) == (run["status"][a], run["iters"][a], run["n_inl"][a]), (o, s[o])
            worst = max(worst, float(np.abs(Td[o] - run["T"][a]).max()), abs(float(s["rmse"][o]) - run["rmse"][a]))
            assert s["fitness"][o] == run["fitness"][a], (o, s["fitness"][o], run["fitness"][a])
        print(f"   chain scene: {len(slots)} candidates, {int(run['accepted'].sum())} accepted, |T - icp_np| <= {worst:.2e} (bound {ICP_TOL:.0e})")
        assert worst <= ICP_TOL
        assert np.array_equal(host(accepted)[slots], run["accepted"])                          # the accepted set equals the restatement's
        model = pg.PoseGraphModel(EC)                                # the log of the device's own T: what the gate and the relaxation read
        want_info = px.add_batch(model, res["pair_dst"], res["pair_src"], Td, host(accepted), None, *c["w"])
        assert host(info).tolist() == want_info.tolist()
        for nm in api.PoseGraph.NAMES:
            assert same_bytes(host(getattr(log, nm)), getattr(model, nm)), nm
        tabs = gate_np.default_tables(c["gate"]["max_gap"])
        kept = pg.PoseGraphModel(EC)
        gw = gate_np.gate(sc["est"], n, model, n, rot_tab=tabs[0], trans2_tab=tabs[1], dst=kept, margins=True, **c["gate"])
        assert gw["margin"] > 1e-6 and np.array_equal(host(keep), gw["keep"]) and host(ginfo).tolist() == gw["info"].tolist()
        assert gw["info"][1] >= 0.9 * model.state[0]

        def fn(case, **kw):
            return pg.relax(sc["est"], n, kept.edge_ij, kept.edge_Z, kept.edge_w, kept.state[0], **dict(c["relax"], **kw))
        a, ra, tol, rtol = bound(None, fn)
        got = host(relaxed)
        print(f"   relaxed poses: |device - posegraph_np| = {np.abs(got - a).max():.2e} (bound {tol:.2e})")
        assert np.abs(got - a).max() <= tol and np.abs(host(report)[:len(ra)] - ra).max() <= rtol
        before, after = centre_error(sc["est"], sc["gt"]), centre_error(got, sc["gt"])
        print(f"   largest centre error {before:.3f} m -> {after:.3f} m")
        assert after < 0.5 * before
        # search -> refine -> select -> add_batch captured once and replayed over two query ranges
        step_log = api.PoseGraph(ctx, n, EC)
        eager_log = api.PoseGraph(ctx, n, EC)
        outs = [ps.search_map(km, qr, **c["search"]) for _ in range(2)]
        infos = [torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(2)]

        def step(lg, out, vout, inf):
            cd = ps.search_map(km, qr, log=lg, known_window=1, out=out, **c["search"])
            Tv, _, ac = ps.verify_map_torch(km, cd, 1024, min_fitness=c["min_fitness"], max_rmse=c["max_rmse"], out=vout, **c["icp"])
            lg.add_batch_torch(cd.pair_dst, cd.pair_src, Tv, ac, None, *c["w"], info=inf)

        step(eager_log, outs[0], None, infos[0])                     # sizes the context's ICP scratch; its buffers serve the eager runs
        vouts = [ps.last_verify, None]
        eager_log.reset()
        step(step_log, outs[1], None, infos[1])
        vouts[1] = ps.last_verify
        step_log.reset()
        ctx.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step(step_log, outs[1], vouts[1], infos[1])
        step_log.reset()
        ctx.sync()
        for rng_ in ((0, 50), (40, 40)):                             # the second range meets pairs the first one logged: known = 1
            qr.copy_(torch.tensor(rng_, dtype=torch.int32))
            graph.replay()
            step(eager_log, outs[0], vouts[0], infos[0])
            st.synchronize()
            for nm in api.PoseGraph.NAMES:
                assert same_bytes(host(getattr(step_log, nm)), host(getattr(eager_log, nm))), (rng_, nm)
            for nm in NAMES:
                assert same_bytes(host(getattr(outs[1], nm)), host(getattr(outs[0], nm))), (rng_, nm)
        assert int(host(outs[0].info)[2]) > 0 and int(host(infos[0])[2]) > 20
        del graph
        for x in (gate, step_log, eager_log, log, dst, ps, km):
            x.close()
        ctx.close()


def bound(case, fn, **kw):
    """test_gpu_posegraph.py's bound(): 100 x the restatement against itself in the other order of the sums, floored at 100 roundings of the
    largest pose entry"""
    a, ra = fn(case, **kw)
    b, rb = fn(case, reverse=True, pairwise=True, **kw)
    d = np.abs(a - b)
    floor = 100 * EPS * max(1.0, float(np.abs(a).max(initial=0.0)))
    rfloor = 100 * EPS * max(1.0, float(np.abs(ra).max(initial=0.0)))
    return a, ra, max(100 * float(d.max(initial=0.0)), floor), max(100 * float(np.abs(ra - rb).max(initial=0.0)), rfloor)


def centre_error(P, gt):
    c = lambda X: -np.einsum("nji,nj->ni", X.reshape(-1, 3, 4)[:, :, :3], X.reshape(-1, 3, 4)[:, :, 3])
    return float(np.linalg.norm(c(np.asarray(P)) - c(gt), axis=1).max())
