"""The loop-closure log and the pose-graph relaxation on the device (pr_posegraph, posegraph.hip) against the NumPy
restatement (posegraph_np.py).

add: integers and copied doubles bit-equal to the restatement, guard words behind all four buffers.

relax, tolerances - never taken from the device's output:
  * noisy graphs (12 nodes / 3 closures, 40 / 4; weights 100 / 10, lambda 1e-9, outer 10, inner 6 n - budgets at which the restatement's
    cost is stationary: 0.45857 and 0.70458 from the fourth step on): 100 x the largest difference between the restatement and itself
    with the per-node edge order reversed and the dot products summed pairwise.  Measured on a CPU (posegraph_np.SELF_POSE /
    SELF_REPORT): poses 6.4e-15 / 2.2e-14, report 7.1e-15 / 3.4e-13 - so the bounds are 6.4e-13 / 2.2e-12 and 7.1e-13 / 3.4e-11.
  * consistent graph: 100 x the restatement's own error against ground truth on the committed case, 8.9e-15 -> 8.9e-13.
  * the count sweep and the drive: the same rule, the self-difference measured when the test runs (bound()), with a floor of 100
    roundings of the largest pose entry (the device's libm and 3 x 3 products round differently from NumPy's even where the restatement's
    two orders agree to the bit, as they do for two or three nodes).  The sweep runs outer 4, inner min(6 n, 600).  Up to 40 nodes that
    leaves the restatement's cost stationary.  At 257 nodes it does NOT: 600 iterations truncate the inner solve and the cost still falls
    by about 1 % per step (e.g. 4.4e-3 -> 3.99e-3 -> 3.96e-3 -> 3.95e-3 with one closure).  The budget is kept there because a fixed
    iteration count far past convergence divides rounding noise by rounding noise: at inner = 1542 the restatement's two orders agree
    only to 7e-4, at 600 to 1e-12, so the bound (at most 1.4e-10 over the four 257-node cases) stays tight."""
import numpy as np
import pytest
import torch

import posegraph_np as pg
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_online import KCAP, MAXC, PCAP, STEP_K, STEP_MASK, pose_inputs, same_bytes, seq07  # noqa: F401  (seq07: the drive's fixture)

pytestmark = pytest.mark.gpu

OVERFLOW = _lib.POSEGRAPH_OVERFLOW
GUARD = -7
EPS = 2.0 ** -52


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def host(t):
    return t.cpu().numpy()


def bound(case, fn, **kw):
    """100 x the restatement against itself in the other order of the sums, floored at 100 roundings of the largest pose entry"""
    a, ra = fn(case, **kw)
    b, rb = fn(case, reverse=True, pairwise=True, **kw)
    fin = np.isfinite(a) & np.isfinite(b)                           # (a non-finite input row passes through; it is compared by its bytes)
    d = np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0))
    floor = 100 * EPS * max(1.0, float(np.abs(a[fin]).max(initial=0.0)))
    rfloor = 100 * EPS * max(1.0, float(np.abs(ra).max(initial=0.0)))
    return a, ra, max(100 * float(d.max(initial=0.0)), floor), max(100 * float(np.abs(ra - rb).max(initial=0.0)), rfloor)


# ------------------------------------------------------------------------------------------------ 1. add
def guarded(ctx, cap, node_capacity=16):
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


def assert_log(g, model, what):
    for n in api.PoseGraph.NAMES:
        assert same_bytes(host(getattr(g, n)), getattr(model, n)), (what, n)


def slots(count):
    """count slots that walk through every combination of accepted 0 / 1, idx -1 / valid / the query's row, and a NaN in T: one in
    twelve is logged"""
    rng = np.random.default_rng(count)
    acc, kind, nan = np.zeros(count, np.uint8), np.zeros(count, np.int64), np.zeros(count, bool)
    for s in range(count):
        c = (s * 5) % 12                               # (5 and 12 are coprime: a walk through all twelve)
        acc[s], kind[s], nan[s] = c % 2, (c // 2) % 3, c // 6
    T = rng.random((count, 12))
    T[nan, rng.integers(0, 12, count)[nan]] = np.nan
    return acc, kind, T


@pytest.mark.parametrize("k", [1, 5, 128])
def test_add_equals_the_restatement(k):
    CAP = 3
    ctx = _stream_context(0)
    g, intact, big = guarded(ctx, CAP)
    h = api.PoseGraph(ctx, 16, CAP)                    # the host form on a second graph
    model = pg.PoseGraphModel(CAP)
    calls = {1: 50, 5: 10, 128: 2}[k]                  # 50 .. 256 slots: 4 or more logged, the count walks 0 .. CAP - 1, CAP, and overflows
    acc, kind, T = slots(calls * k)
    seen = set()
    for c in range(calls):
        sl = slice(c * k, (c + 1) * k)
        row = 40 + c
        idx = np.where(kind[sl] == 0, -1, np.where(kind[sl] == 1, np.arange(k) % 30, row)).astype(np.int32)
        qr = torch.tensor([row, GUARD], dtype=torch.int32, device="cuda")
        info = g.add_torch(dev(idx, np.int32)[None], dev(T[sl]).reshape(1, k, 3, 4), dev(acc[sl], np.uint8)[None], qr[:1], 2.0 + c, 0.5, None)
        want = model.add(idx, T[sl], acc[sl], row, 2.0 + c, 0.5)
        ctx.sync()
        assert host(info).tolist() == want.tolist(), (c, host(info), want)
        assert_log(g, model, c)
        intact()
        assert h.add(idx, T[sl], acc[sl], row, 2.0 + c, 0.5).tolist() == want.tolist(), c
        assert_log(h, model, ("host", c))
        seen.add(int(want[2]))
    assert CAP in seen and (k == 128 or CAP - 1 in seen) and model.state.tolist() == [CAP, OVERFLOW, 0, 0] and g.count() == (CAP, OVERFLOW)
    # a negative query row changes no byte (the scribbled count of the next step included)
    before = {n: host(t).copy() for n, t in big.items()}
    off = torch.tensor([-1], dtype=torch.int32, device="cuda")
    info = g.add_torch(dev(np.arange(k), np.int32), dev(np.ones((k, 12))), dev(np.ones(k), np.uint8), off, 1.0, 1.0)
    ctx.sync()
    assert host(info).tolist() == [0, -1, CAP, OVERFLOW] == model.add(np.arange(k), np.ones((k, 12)), np.ones(k), -1).tolist()
    assert all(same_bytes(host(big[n]), before[n]) for n in big)
    # a scribbled count is clamped before it forms an address
    g.state[0] = 1 << 30; model.state[0] = 1 << 30
    info = g.add_torch(dev(np.arange(k), np.int32), dev(np.ones((k, 12))), dev(np.ones(k), np.uint8), dev([50], np.int32), 1.0, 1.0)
    ctx.sync()
    assert host(info).tolist() == model.add(np.arange(k), np.ones((k, 12)), np.ones(k), 50).tolist() == [0, -1, CAP, OVERFLOW]
    intact()
    g.reset(); model.reset()
    ctx.sync()
    assert g.count() == (0, 0) and not host(g.state).any()
    info = g.add_torch(dev([4], np.int32), dev(np.ones((1, 12))), dev([1], np.uint8), dev([9], np.int32), 1.0, 1.0)
    ctx.sync()
    assert host(info).tolist() == model.add([4], np.ones((1, 12)), [1], 9).tolist() == [1, 0, 1, 0]
    assert_log(g, model, "after reset")
    intact()
    with pytest.raises(_lib.PRError, match="k=129"):
        g.add_torch(dev(np.zeros(129), np.int32), dev(np.ones((129, 12))), dev(np.ones(129), np.uint8), off)
    g.close(); h.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. relax: the count sweep
def load_log(g, case, ctx):
    """the case's edges through the host form, one add per edge (the restatement's log_of)"""
    w = case.get("w", (1.0, 1.0))
    for (i, j), Z in zip(case["pairs"], case["Z"]):
        g.add([i], Z, [1], j, *w)


def run_relax(g, poses, n, params, out=None):
    N = g.node_capacity
    buf = torch.full((N + 2, 12), float(GUARD), dtype=torch.float64, device="cuda")          # two guard rows behind the capacity
    buf[:len(poses)] = dev(poses)
    o = torch.full((N + 2, 12), float(GUARD), dtype=torch.float64, device="cuda") if out is None else out
    nd = torch.tensor([n, GUARD, GUARD, GUARD], dtype=torch.int32, device="cuda")
    rep = torch.full((params["outer"] + 3,), float(GUARD), dtype=torch.float64, device="cuda")
    g.relax_torch(buf[:N], nd, out=o[:N], report=rep[:params["outer"] + 2], **params)
    g.ctx.sync()
    assert host(rep)[-1] == GUARD and (host(o)[N:] == GUARD).all()
    return host(o)[:N], host(rep)[:-1]


SWEEP = [(n, log) for n in pg.SWEEP_NODES for log in pg.SWEEP_LOGS]


@pytest.mark.parametrize("n,log", SWEEP)
def test_relax_equals_the_restatement_over_node_and_edge_counts(n, log):
    c = pg.sweep_case(n, log)
    want, wrep, tol, rtol = bound(c, pg.relax_sweep)
    N = n + 3                                          # node_capacity > n: the rows behind n keep their bytes
    ctx = _stream_context(0)
    g = api.PoseGraph(ctx, N, 8, max_outer=4, max_inner=600)
    load_log(g, c, ctx)
    got, rep = run_relax(g, c["poses"], n, c["params"])
    dp = float(np.abs(got[:n] - want[:n]).max(initial=0.0))
    dr = float(np.abs(rep - wrep).max())
    print(f"   n {n} log {log}: cost {wrep[:-1].tolist()} |pose - model| {dp:.2e} (bound {tol:.2e}) |report - model| {dr:.2e} (bound {rtol:.2e})")
    assert (got[n:] == GUARD).all()                    # rows >= n are not written
    assert rep[-1] == wrep[-1]                         # edges used
    assert dp <= tol and dr <= rtol
    if n < 2 or log == "none":
        assert same_bytes(got[:n], c["poses"][:n]) and not rep[:-1].any()      # nothing to relax: the input's bytes
    else:
        assert same_bytes(got[0], c["poses"][0])       # the gauge
    with pytest.raises(_lib.PRError, match="max_outer"):
        g.relax_torch(torch.zeros((N, 12), dtype=torch.float64, device="cuda"), g.state, outer=5, inner=1)
    with pytest.raises(_lib.PRError, match="max_inner"):
        g.relax_torch(torch.zeros((N, 12), dtype=torch.float64, device="cuda"), g.state, outer=1, inner=601)
    g.close(); ctx.close()


def test_relax_passes_negative_zero_and_non_finite_rows_through():
    c = pg.sweep_case(12, "four")
    poses = c["poses"].copy()
    poses[7, 3] = np.inf                               # node 7 loses its edges and keeps its bytes
    c = dict(c, poses=poses)
    want, wrep, tol, rtol = bound(c, pg.relax_sweep)
    ctx = _stream_context(0)
    g = api.PoseGraph(ctx, 15, 8, max_outer=4, max_inner=600)
    load_log(g, c, ctx)
    got, rep = run_relax(g, poses, 12, c["params"])
    ok = np.isfinite(want[:12])
    assert same_bytes(got[7], poses[7]) and np.array_equal(np.isfinite(got[:12]), ok) and rep[-1] == wrep[-1]
    assert np.abs(np.where(ok, got[:12], 0.0) - np.where(ok, want[:12], 0.0)).max() <= tol and np.abs(rep - wrep).max() <= rtol
    g.reset()                                          # an empty log: a negative zero survives
    poses = c["poses"].copy()
    poses[4, 2] = -0.0
    poses[7, 3] = 1.0
    got, rep = run_relax(g, poses, 12, c["params"])
    assert same_bytes(got[:12], poses[:12]) and rep.tolist() == [0.0] * 5 + [11.0]
    g.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the consistent graph
def test_the_consistent_graph_recovers_ground_truth():
    c = pg.consistent_case()
    ctx = _stream_context(0)
    g = api.PoseGraph(ctx, 12, 32, max_outer=6, max_inner=72)
    load_log(g, c, ctx)
    got, rep = run_relax(g, c["poses"], 12, c["params"])
    err = float(np.abs(got - c["gt"]).max())
    print("   consistent graph: cost", rep[:-1].tolist(), "max |pose - truth|", err, "(restatement:", pg.CONSISTENT_ERR, ")")
    assert rep[-1] == 28 and rep[0] > 1.0
    assert err <= 100 * pg.CONSISTENT_ERR              # = 8.9e-13
    g.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. noisy graphs
@pytest.fixture(scope="module")
def noisy_refs():
    """the restatement of the two noisy cases, computed once"""
    out = {}
    for n, k, seed in ((12, 3, 1), (40, 4, 2)):
        c = pg.noisy_case(n, k, seed)
        out[n] = (c,) + pg.relax_case(c)
    return out


@pytest.mark.parametrize("n", [12, 40])
def test_noisy_graphs_equal_the_restatement(noisy_refs, n):
    c, want, wrep = noisy_refs[n]
    ctx = _stream_context(0)
    g = api.PoseGraph(ctx, n, 8, max_outer=10, max_inner=6 * n)
    load_log(g, c, ctx)
    got, rep = run_relax(g, c["poses"], n, c["params"])
    dp, dr = float(np.abs(got - want).max()), float(np.abs(rep - wrep).max())
    print(f"   n {n}: cost {rep[:-1].tolist()} |pose - model| {dp:.2e} (bound {100 * pg.SELF_POSE[n]:.2e}) |report - model| {dr:.2e} "
          f"(bound {100 * pg.SELF_REPORT[n]:.2e})")
    assert rep[-1] == wrep[-1] == n - 1 + len(c["pairs"])
    assert dp <= 100 * pg.SELF_POSE[n] and dr <= 100 * pg.SELF_REPORT[n]
    g.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_two_runs_in_place_and_one_capture_for_every_count(noisy_refs):
    c = noisy_refs[40][0]
    prm = dict(c["params"], outer=3, inner=60)
    N = 44
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        g = api.PoseGraph(ctx, N, 8, max_outer=3, max_inner=60)
        poses = torch.zeros((N, 12), dtype=torch.float64, device="cuda")
        poses[:40] = dev(c["poses"])
        nd = torch.zeros(4, dtype=torch.int32, device="cuda")                # a map's state: word 0 is the count - 0 at the capture
        out = torch.zeros((N, 12), dtype=torch.float64, device="cuda")
        rep = torch.zeros(5, dtype=torch.float64, device="cuda")
        g.relax_torch(poses, nd, out=out, report=rep, **prm)                 # one eager call, then the capture of the same call
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            g.relax_torch(poses, nd, out=out, report=rep, **prm)
        w = c["w"]
        moved = 0
        for n, edges in ((12, 1), (40, 2), (33, 4)):                         # three node and edge counts under the one capture
            while g.count()[0] < edges:
                e = g.count()[0]
                g.add([c["pairs"][e][0]], c["Z"][e], [1], c["pairs"][e][1], *w)
            nd[0] = n
            out.fill_(GUARD); rep.fill_(GUARD)
            graph.replay()
            st.synchronize()
            a, ra = host(out).copy(), host(rep).copy()
            o2, r2 = g.relax_torch(poses, nd, **prm)                         # eager, fresh buffers
            o3, r3 = g.relax_torch(poses, nd, **prm)                         # and again
            work = poses.clone()
            g.relax_torch(work, nd, out=work, report=torch.zeros(5, dtype=torch.float64, device="cuda"), **prm)      # in place
            st.synchronize()
            assert same_bytes(a[:n], host(o2)[:n]) and same_bytes(ra, host(r2)), (n, edges)
            assert same_bytes(host(o2), host(o3)) and same_bytes(host(r2), host(r3)), (n, edges)
            assert same_bytes(host(work)[:n], a[:n]) and same_bytes(host(work)[n:], host(poses)[n:]), (n, edges)
            assert (a[n:] == GUARD).all() and ra[-1] == n - 1 + sum(1 for i, j in c["pairs"][:edges] if i < n and j < n)
            moved += int(not same_bytes(a[:n], host(poses)[:n]))
        assert moved >= 2                                                    # the replays did relax something
        del graph
        g.close(); ctx.close()


def test_null_pointers_on_a_live_handle_are_refused():
    import ctypes as C
    ctx = _stream_context(0)
    g = api.PoseGraph(ctx, 8, 4)
    lib, P = ctx.lib, _lib.PR_EINVAL
    buf = torch.zeros(8 * 12 + 16, dtype=torch.float64, device="cuda")
    d = C.c_void_p(buf.data_ptr())
    n, f = C.c_int32(), C.c_int32()
    err = lambda: lib.pr_last_error(ctx.h)
    for who in range(5):                               # d_idx, d_T, d_accepted, d_query_row, d_info
        a = [d, d, d, d, d]
        a[who] = None
        assert lib.pr_posegraph_add_dev(g.h, a[0], a[1], a[2], a[3], 1, 1.0, 1.0, a[4]) == P and b"pr_posegraph_add_dev: a required pointer is NULL" in err()
    hb = (C.c_double * 16)()
    for who in range(4):                               # idx, T, accepted, info (host)
        a = [hb, hb, hb, hb]
        a[who] = None
        assert lib.pr_posegraph_add(g.h, a[0], a[1], a[2], 3, 1, 1.0, 1.0, a[3]) == P and b"pr_posegraph_add: a required pointer is NULL" in err()
    prm = _lib.PoseGraphParams(1, 1, 0.0, 1.0, 1.0)
    for who in range(4):                               # d_poses_in, d_n, d_poses_out, d_report
        a = [d, d, d, d]
        a[who] = None
        assert lib.pr_posegraph_relax_dev(g.h, a[0], a[1], C.byref(prm), a[2], a[3]) == P and b"pr_posegraph_relax_dev: a required pointer is NULL" in err()
    assert lib.pr_posegraph_relax_dev(g.h, d, d, None, d, d) == P and b"params is NULL" in err()
    assert lib.pr_posegraph_count(g.h, None, C.byref(f)) == P and b"pr_posegraph_count: a required pointer is NULL" in err()
    assert lib.pr_posegraph_count(g.h, C.byref(n), None) == P and b"pr_posegraph_count: a required pointer is NULL" in err()
    ctx.sync()
    assert g.count() == (0, 0) and not host(buf).any()                       # nothing ran
    g.close(); ctx.close()


def test_pose_graph_and_map_must_share_one_context():
    ctx, other = _stream_context(0), _stream_context(0)
    km = api.KeyframeMap(other, 8, 64, 16)
    g = api.PoseGraph(ctx, 8, 4)
    with pytest.raises(ValueError, match="share one context"):
        g.relax_map(km)
    km.close(); g.close(); other.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the drive
DRIVE = dict(outer=5, inner=220, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
DRIVE_W = (100.0, 10.0)


def run_drive(drive, captured):
    """the online step of test_gpu_online.run_drive with pg.add_torch behind the verify: eagerly, or as ONE graph captured behind the first
    eager step.  Returns per pose the host copies of idx, T, accepted and the map append's info, and - read after the drive - the log,
    the map's poses and state, and relax_map's result."""
    P = len(drive["pid"])
    res = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        lib = ctx.lib
        p = lambda t: t.data_ptr()
        pose = torch.zeros(12, dtype=torch.float64, device="cuda"); x = torch.zeros((60, 3), dtype=torch.float64, device="cuda")
        it = torch.zeros(60, dtype=torch.float32, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        kid = torch.zeros(1, dtype=torch.int32, device="cuda")
        sig = torch.zeros((1, 2400), dtype=torch.float64, device="cuda")
        mout = (torch.zeros((1, STEP_K), dtype=torch.int32, device="cuda"), torch.zeros((1, STEP_K), dtype=torch.float64, device="cuda"))
        oinfo = torch.zeros(4, dtype=torch.int32, device="cuda"); minfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        ginfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
        km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
        odb = api.OnlineDatabase(ctx, "sc", KCAP, max_k=STEP_K)
        graph_log = api.PoseGraph(ctx, KCAP, 2 * KCAP)
        out = win.empty_out()
        keep = dict(al=None, v=None)

        def load(i):
            w, hx, hit, k, pid = pose_inputs(drive, i)
            pose.copy_(torch.from_numpy(w.copy())); x.copy_(torch.from_numpy(hx)); it.copy_(torch.from_numpy(hit))
            n.fill_(k); kid.fill_(pid)

        def step():
            win.push_torch(pose, x, it, n, out=out)
            ctx.check(lib.pr_sc_generate_frames_dev(ctx.h, p(out["xyz"]), p(out["inten"]), p(out["offs"]), 1, 45.0, p(out["frame"]), 1, p(sig)))
            odb.step_torch(sig, STEP_MASK, 2.0, STEP_K, emitted=out["info"], out=mout, info=oinfo)
            km.append_push(out, pose=pose, id=kid, info=minfo)
            keep["al"] = odb.align(mout[0], sig, out=keep["al"])
            keep["v"] = km.verify_variants("sc", mout[0], keep["al"][0], (out["xyz"], out["offs"]), out["frame"][None], 9000, hypotheses=2,
                                           max_corr=1.0, min_fitness=0.5, max_rmse=0.5, max_iter=10, out=keep["v"])
            graph_log.add_torch(mout[0], keep["v"][0], keep["v"][2], minfo[1:2], *DRIVE_W, info=ginfo)

        g = None
        for i in range(P):
            load(i)
            if g is not None:
                g.replay()
            else:
                step()
                if captured:
                    st.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        step()
            st.synchronize()
            T, stats, acc, hyp = keep["v"]
            res.append(dict(idx=host(mout[0]), T=host(T), accepted=host(acc), map_info=host(minfo), log_info=host(ginfo)))
        log = {nm: host(getattr(graph_log, nm)).copy() for nm in api.PoseGraph.NAMES}
        poses, state = host(km.poses).copy(), host(km.state).copy()
        corrected = torch.full((KCAP, 12), float(GUARD), dtype=torch.float64, device="cuda")
        _, rep = graph_log.relax_map(km, out=corrected, **DRIVE)
        st.synchronize()
        relaxed = (host(corrected).copy(), host(rep).copy())
        assert same_bytes(host(km.poses), poses)                             # out= elsewhere: the map's own poses are not touched
        del g
        graph_log.close(); odb.close(); km.close(); win.close(); ctx.close()
    return res, log, poses, state, relaxed


def test_the_drive_logs_its_closures_in_the_graph_and_relaxes_the_map(seq07):
    got, glog, gposes, gstate, (corrected, rep) = run_drive(seq07, captured=True)
    want, wlog, wposes, wstate, (wcorrected, wrep) = run_drive(seq07, captured=False)
    # the log of the captured drive = the host-side filter of the eager loop's per-keyframe (idx, T, accepted)
    model = pg.PoseGraphModel(2 * KCAP)
    for i, (a, b) in enumerate(zip(got, want)):
        info = model.add(b["idx"], b["T"], b["accepted"], int(b["map_info"][1]), *DRIVE_W)
        assert a["log_info"].tolist() == b["log_info"].tolist() == info.tolist(), (i, a["log_info"], info)
    for nm in api.PoseGraph.NAMES:
        assert same_bytes(glog[nm], getattr(model, nm)) and same_bytes(wlog[nm], getattr(model, nm)), nm
    assert same_bytes(gposes, wposes) and gstate.tolist() == wstate.tolist() == [110, 0, 0, 0]
    assert same_bytes(corrected, wcorrected) and same_bytes(rep, wrep)
    edges = int(model.state[0])
    # relax_map against the restatement, within the bound of the restatement against itself (no property of the cost is asserted: the
    # step has no line search and the drive's closures carry ICP error)
    case = dict(poses=gposes)
    fn = lambda c, **kw: pg.relax(c["poses"], 110, model.edge_ij, model.edge_Z, model.edge_w, edges, **dict(DRIVE, **kw))
    m_poses, m_rep, tol, rtol = bound(case, fn)
    dp, dr = float(np.abs(corrected[:110] - m_poses[:110]).max()), float(np.abs(rep - m_rep).max())
    print(f"   the drive: {edges} closures logged, cost {rep[:-1].tolist()}, |pose - model| {dp:.2e} (bound {tol:.2e}) "
          f"|report - model| {dr:.2e} (bound {rtol:.2e})")
    assert (corrected[110:] == GUARD).all() and rep[-1] == m_rep[-1]
    assert dp <= tol and dr <= rtol
