"""The registration information on the device (pr_reginfo, reginfo.hip; pr_posegraphw_add) against the NumPy
restatement (reginfo_np.py).

  stat, ok     exactly.
  H, SSE       a derived bound.  The device's terms are the restatement's bits (the same association, no contraction); only the order of
               the additions may differ, so per entry |dev - restatement| <= 2 ns 2^-53 sum |term| - the bound of two sums of ns terms in
               any two orders -, propagated through the assembly of H (one more rounding of the entry).  The restatement adds in the
               device's order, so in practice the difference is zero; the bound is what is asserted.
  cov, spec, w a measured bound: 100 x |restatement in the kernel's order - restatement with the sums reversed and the inverse and the
               eigen-decompositions in mpmath|, per slot and array, floored at 100 roundings of the array's largest entry, taken when
               the test runs and never from the device; only for slots whose cond(H) <= 1e8 (test_reginfo_cpu.py holds every compared
               slot to it).  Flagged slots compare flags, zeros and w == 0.0 exactly.
Guard words stand behind every output.  The chunk partials lie inside the handle's own allocation, which no public call exposes: what
stands behind them is not checked here (their extent is the header's formula, test_reginfo_cpu.py)."""
import numpy as np
import pytest
import torch

import posegraph_np as pg
import reginfo_np as rn
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_online import KCAP, MAXC, PCAP, STEP_K, STEP_MASK, pose_inputs, same_bytes, seq07  # noqa: F401  (seq07: the drive's fixture)
from test_gpu_posegraph import bound, guarded

pytestmark = pytest.mark.gpu

GUARD = -7.0
EPS = 2.0 ** -52
FIELDS = api.RegInfo._fields


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def host(t):
    return t.cpu().numpy()


class Rig:
    """a handle, the case's inputs on the device and guarded outputs (one row more than c, filled with a guard pattern)"""

    def __init__(self, case, plane, prm):
        self.case, self.plane, self.prm = case, plane, prm
        self.ctx = _stream_context(0)
        self.c = len(case["src"])
        self.ri = api.RegistrationInfo(self.ctx, self.c, case["max_src_pts"])
        self.xq, self.oq = dev(case["xq"]), dev(case["oq"], np.int64)
        self.src, self.T, self.acc = dev(case["src"], np.int32), dev(case["T"]), dev(case["acc"], np.uint8)
        self.nn = (dev(case["nn"][0], np.int64), dev(case["nn"][1], np.int32), dev(case["nn"][2]))
        if plane:
            self.world, self.normals, self.ninfo = dev(case["world"]), dev(case["normals"]), dev(case["ninfo"], np.int32)

    def run(self, rows=None, oc=None, **kw):
        """the device form over the slots `rows` (default: all); returns host arrays"""
        rows = list(range(self.c)) if rows is None else rows
        c = len(rows)
        src, T, acc = self.src[rows].contiguous(), self.T[rows].contiguous(), self.acc[rows].contiguous()
        offs = host(self.nn[0])
        spans = [int(offs[p + 1] - offs[p]) for p in rows]
        oo = np.concatenate([[0], np.cumsum(spans)]).astype(np.int64)
        pick = np.concatenate([np.arange(offs[p], offs[p + 1]) for p in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        pick = torch.from_numpy(pick).cuda()
        nn = (dev(oo, np.int64), self.nn[1][pick].contiguous(), self.nn[2][pick].contiguous())
        big = [torch.full((c + 1,) + s, GUARD, dtype=torch.float64, device="cuda") for s in ((6, 6), (6, 6), (16,), (2,))]
        big += [torch.full((c + 1, 4), int(GUARD), dtype=torch.int32, device="cuda"), torch.ones(c + 1, dtype=torch.bool, device="cuda")]
        out = api.RegInfo(*(b[:c] for b in big))
        prm = dict(self.prm, **kw)
        if self.plane:
            oc = len(self.case["world"]) if oc is None else oc
            got = self.ri.plane_torch(self.xq, self.oq, src, T, nn, self.world[:oc], self.normals[:oc], self.ninfo[:oc], acc, out=out, **prm)
        else:
            got = self.ri.point_torch(self.xq, self.oq, src, T, nn, acc, out=out, **prm)
        self.ctx.sync()
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        for b in big[:4]:
            assert bool((b[c:] == GUARD).all())
        assert bool((big[4][c:] == int(GUARD)).all()) and bool(big[5][c])
        return {k: host(t).copy() for k, t in zip(FIELDS, got)}

    def run_host(self):
        cs = self.case
        args = (cs["xq"], cs["oq"], cs["src"], cs["T"], cs["nn"])
        if self.plane:
            r = self.ri.plane(*args, cs["world"], cs["normals"], cs["ninfo"], accepted=cs["acc"], **self.prm)
        else:
            r = self.ri.point(*args, accepted=cs["acc"], **self.prm)
        return dict(zip(FIELDS, r))

    def close(self):
        self.ri.close(); self.ctx.close()


def h_bound(plane, terms, H):
    """|dev - restatement| of H [6, 6] and of SSE: 2 ns 2^-53 sum |term| per sum, through the assembly, plus the entry's own rounding"""
    b = 2.0 * len(terms) * 2.0 ** -53 * np.abs(terms).sum(axis=0)
    sse = b[3] if plane else b[1]
    b[0] = 0.0                                                     # the counts are exact
    if plane:
        b[2] = 0.0
    Hb, _, _, _, _ = rn.assemble(plane, b)
    return np.abs(np.array(Hb)) + 2.0 ** -52 * np.abs(H), sse


def check(case, plane, prm, got, want, what):
    """got: the device's arrays; want: run(..., detail=True) of the restatement"""
    assert np.array_equal(got["stat"], want["stat"]), (what, np.nonzero((got["stat"] != want["stat"]).any(axis=1))[0])
    assert np.array_equal(got["ok"], want["ok"]) and np.array_equal(got["ok"], got["stat"][:, 3] == 0)
    compared = 0
    for p, name in enumerate(case["names"]):
        f = int(want["stat"][p, 3])
        if f & (rn.OFF | rn.NONFINITE):
            assert not got["H"][p].any() and not got["spec"][p].any(), (what, name)
        else:
            Hb, sb = h_bound(plane, want["terms"][p], want["H"][p])
            assert (np.abs(got["H"][p] - want["H"][p]) <= Hb).all(), (what, name, "H")
            assert abs(got["spec"][p, 12] - want["spec"][p, 12]) <= sb, (what, name, "SSE")
            assert np.array_equal(got["H"][p], got["H"][p].T)
        if f & ~(rn.WEAK_ROT | rn.WEAK_TRANS):                     # the rule stopped early: zeros, exactly
            assert not got["cov"][p].any() and not got["w"][p].any() and not got["spec"][p, :12].any() and not got["spec"][p, 13:].any(), (what, name)
            continue
        if f:
            assert got["w"][p].tobytes() == np.zeros(2).tobytes(), (what, name)                   # exactly +0.0
        assert np.linalg.cond(want["H"][p]) <= rn.COND_MAX, (what, name)
        m = rn.finish_mp(plane, rn.reversed_sum(want["terms"][p]), prm["min_ratio"], prm["sigma_min"], prm["w_max"])
        assert m["flags"] == f
        for k in ("cov", "spec", "w"):
            a, b, g = want[k][p], m[k], got[k][p]
            tol = max(100.0 * float(np.abs(a - b).max()), 100.0 * EPS * float(np.abs(a).max()))
            err = float(np.abs(g - a).max())
            assert err <= tol, (what, name, k, err, tol)
        compared += 1
    return compared


# ------------------------------------------------------------------------------------------------ 1. the two metrics
@pytest.fixture(scope="module")
def point():
    case = rn.point_case()
    return case, rn.run_point_case(case, detail=True), rn.run_point_case(case, detail=True, w_max=50.0)


@pytest.fixture(scope="module")
def plane():
    case = rn.plane_case()
    return case, rn.run_plane_case(case, detail=True)


def test_point_metric_sizes_edges_and_run_forms(point):
    case, want, capped = point
    rig = Rig(case, 0, rn.POINT)
    got = rig.run()
    n = check(case, 0, rn.POINT, got, want, "point")
    assert n >= 13
    again = rig.run()
    assert all(same_bytes(got[k], again[k]) for k in FIELDS)                                       # two runs: the same bytes
    hostf = rig.run_host()
    assert all(same_bytes(got[k], np.asarray(hostf[k]).reshape(got[k].shape)) for k in FIELDS)    # the host form is the device form
    got50 = rig.run(w_max=50.0)
    check(case, 0, dict(rn.POINT, w_max=50.0), got50, capped, "point, w_max = 50")
    assert (got50["w"][got50["ok"]] == 50.0).all()
    # c = 1 / 3 / 5: a slot's bytes do not depend on the other slots of the call
    names = case["names"]
    box, col, nan = names.index("the 60-point box"), names.index("collinear on an integer grid"), names.index("a NaN in T")
    for rows in ([box], [names.index("size 257"), names.index("pair_src -1"), col], [names.index("size 513"), nan, box, names.index("accepted 0"), 0]):
        sub = rig.run(rows=rows)
        assert all(same_bytes(sub[k], got[k][rows]) for k in FIELDS), rows
    rig.close()


def test_plane_metric_scenes_and_run_forms(plane):
    case, want = plane
    rig = Rig(case, 1, rn.PLANE)
    got = rig.run()
    n = check(case, 1, rn.PLANE, got, want, "plane")
    assert n >= 9
    j = case["names"].index("the jittered corridor")
    assert got["stat"][j, 3] == rn.WEAK_TRANS and got["spec"][j, 9] > 1.0 - 1e-8 and np.abs(got["spec"][j, 10:12]).max() < 1e-3   # dir_t: the axis
    again = rig.run()
    assert all(same_bytes(got[k], again[k]) for k in FIELDS)
    hostf = rig.run_host()
    assert all(same_bytes(got[k], np.asarray(hostf[k]).reshape(got[k].shape)) for k in FIELDS)
    # nn_idx >= out_capacity: with the world cut behind the corner scene the corridors' and the floor's correspondents are no inliers
    oc = case["scene_rows"]
    assert (case["nn"][1] >= oc).any()
    cut = rn.run(1, case["xq"], case["oq"], case["src"], case["T"], case["acc"], case["nn"], case["max_src_pts"], world=case["world"][:oc],
                 normals=case["normals"][:oc], ninfo=case["ninfo"][:oc], detail=True, **rn.PLANE)
    got_cut = rig.run(oc=oc)
    check(case, 1, rn.PLANE, got_cut, cut, "plane, world cut")
    assert got_cut["stat"][j].tolist() == [0, 0, -6, rn.TOO_FEW]
    rows = [case["names"].index(n) for n in ("the corner scene", "one floor", "scene, size 257", "the jittered corridor", "n_pl = 6")]
    for r in (rows[:1], rows[:3], rows):
        sub = rig.run(rows=r)
        assert all(same_bytes(sub[k], got[k][r]) for k in FIELDS), r
    rig.close()


def test_c_zero_and_a_refused_call_touch_nothing(point):
    case = point[0]
    rig = Rig(case, 0, rn.POINT)
    out = rig.run(rows=[])
    assert out["stat"].shape == (0, 4)
    with pytest.raises(api.PRError):
        rig.ri.point_torch(rig.xq, rig.oq, rig.src, rig.T, rig.nn, rig.acc, min_inliers=2)
    rig.close()


def test_maploc_torch_runs_the_localisers_pass_and_the_plane_form():
    """RegistrationInfo.maploc_torch over mapplane's refine world (the corner scene inside a world of capacity 1024): the pass is
    pr_maploc_nn_dev through the voxel index, the normals are the device's; against the restatement fed with maploc_np's search"""
    import icp_np
    import maploc_np as mnp
    import mapplane_np as pnp
    from test_gpu_mapplane import PlaneWorld
    rc = pnp.refine_case()
    ctx = _stream_context(0)
    W = PlaneWorld(ctx, 1024, rc["cell"], 6, 513)
    W.put(rc["xyz"], rc["row"])
    W.ml.index_torch()
    nrm, ninfo = W.pl.normals_torch(**pnp.SCENE_NORMALS)
    ri = api.RegistrationInfo(ctx, 6, 513)
    c = 6                                                          # clouds of 0, 1, 255, 256, 257 and 513 points at the scene's truth
    T = np.tile(rc["truth"], (c, 1, 1))
    ps = np.arange(c, dtype=np.int32)
    got = ri.maploc_torch(W.pl, dev(rc["xq"]), dev(rc["oq"], np.int64), dev(ps, np.int32), dev(T), nrm, ninfo, **rn.PLANE)
    ctx.sync()
    got = {k: host(t) for k, t in zip(FIELDS, got)}
    xyz, row, _ = W.host()
    ix = mnp.index(xyz, len(rc["xyz"]), rc["cell"], 1024)
    spans, idxs, d2s = [], [], []
    for s in range(c):
        P = rc["xq"][rc["oq"][s]:rc["oq"][s + 1]]
        j, d2 = pnp.nn_boxed(ix, xyz, row, icp_np.transform(T[s], P), rn.PLANE["max_corr"]) if len(P) else (np.zeros(0, np.int32), np.zeros(0))
        spans.append(len(P)); idxs.append(j); d2s.append(d2)
    nn = (np.concatenate([[0], np.cumsum(spans)]).astype(np.int64), np.concatenate(idxs).astype(np.int32), np.concatenate(d2s))
    want = rn.run(1, rc["xq"], rc["oq"], ps, T, None, nn, 513, world=xyz, normals=host(nrm), ninfo=host(ninfo), detail=True, **rn.PLANE)
    names = ["size %d" % n for n in pnp.REFINE_SIZES]
    assert check(dict(names=names), 1, rn.PLANE, got, want, "maploc_torch") == 4
    assert got["stat"][:, 3].tolist() == [rn.OFF, rn.TOO_FEW, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="must live on this handle's context"):
        other = _stream_context(0)
        try:
            api.RegistrationInfo.maploc_torch(ri, type("P", (), dict(ctx=other, ml=W.ml))(), dev(rc["xq"]), dev(rc["oq"], np.int64), dev(ps, np.int32),
                                              dev(T), nrm, ninfo)
        finally:
            other.close()
    ri.close(); W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. the weighted add
def _slots(k, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(-1, 30, k).astype(np.int32)
    T = rng.normal(0.0, 1.0, (k, 12))
    acc = (rng.random(k) < 0.8).astype(np.uint8)
    w = np.abs(rng.normal(50.0, 20.0, (k, 2)))
    if k >= 5:
        w[1, 0] = np.nan; w[2, 1] = -1.0; w[3, 0] = np.inf; w[4] = (0.0, -0.0); T[k - 1, 3] = np.nan
    return idx, T, acc, w


@pytest.mark.parametrize("k", [1, 5, 128])
def test_weighted_add_equals_the_restatement(k):
    ctx = _stream_context(0)
    cap = 40 if k < 128 else 150                                   # the adds below run across the capacity
    g, intact, big = guarded(ctx, cap, node_capacity=64)
    m = pg.PoseGraphModel(cap)
    info = torch.zeros(8, dtype=torch.int32, device="cuda"); info[4:] = int(GUARD)
    for q, row in enumerate((31, 32, -1, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43)):
        idx, T, acc, w = _slots(k, 100 * k + q)
        want = rn.add_weighted(m, idx, T, acc, row, w)
        if q % 2:
            got = g.add_weighted(idx, T, acc, row, w)               # the host form
        else:
            g.add_weighted_torch(dev(idx, np.int32), dev(T), dev(acc, np.uint8), torch.tensor([row, 99], dtype=torch.int32, device="cuda"), dev(w),
                                 info=info[:4])
            ctx.sync()
            got = host(info)[:4]
        assert got.tolist() == want.tolist(), (k, q, got, want)
        if k == 128 and m.state[1]:
            break
    for n in api.PoseGraph.NAMES:
        assert same_bytes(host(getattr(g, n)), getattr(m, n)), n
    assert (int(m.state[1]) == pg.OVERFLOW) == (k == 128) and int(m.state[0]) > 0
    assert bool((info[4:] == int(GUARD)).all())
    intact()
    g.close(); ctx.close()


def test_constant_weights_leave_the_bytes_of_add_dev():
    ctx = _stream_context(0)
    a, b = api.PoseGraph(ctx, 64, 20), api.PoseGraph(ctx, 64, 20)
    for q in range(6):
        idx, T, acc, _ = _slots(5, 7 + q)
        T[4, 3] = 0.5
        args = (dev(idx, np.int32), dev(T), dev(acc, np.uint8), torch.tensor([31 + q], dtype=torch.int32, device="cuda"))
        ia = a.add_torch(*args, w_rot=100.0, w_trans=10.0)
        ib = b.add_weighted_torch(*args, dev(np.tile((100.0, 10.0), (5, 1))))
        ctx.sync()
        assert host(ia).tolist() == host(ib).tolist()
    for n in api.PoseGraph.NAMES:
        assert same_bytes(host(getattr(a, n)), host(getattr(b, n))), n
    assert host(a.state)[1] == pg.OVERFLOW
    a.close(); b.close(); ctx.close()


def test_two_contradicting_closures_of_unequal_weight_relax_to_the_restatement():
    """a 12-node circle: the closure (2, 8) measured from ground truth with weight (400, 40) and the same pair once more, 0.3 rad and 1 m
    off, with weight (4, 0.4)"""
    gt = pg.circle_truth(12, 2)
    poses = pg.noisy(gt, 5)
    Z = pg.measure(gt, 2, 8)
    bad = pg.update(Z.reshape(1, 12), np.array([[0.0, 0.0, 0.3, 1.0, 0.0, 0.0]]))[0].reshape(12)
    ctx = _stream_context(0)
    g = api.PoseGraph(ctx, 12, 8)
    m = pg.PoseGraphModel(8)
    idx, T, acc, w = np.array([2, 2], np.int32), np.array([Z, bad]), np.ones(2, np.uint8), np.array([[400.0, 40.0], [4.0, 0.4]])
    assert g.add_weighted(idx, T, acc, 8, w).tolist() == rn.add_weighted(m, idx, T, acc, 8, w).tolist() == [2, 0, 2, 0]
    prm = dict(outer=8, inner=72, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
    out, rep = g.relax_torch(dev(poses), torch.tensor([12], dtype=torch.int32, device="cuda"), **prm)
    ctx.sync()
    fn = lambda c, **kw: pg.relax(c["poses"], 12, m.edge_ij, m.edge_Z, m.edge_w, 2, **dict(prm, **kw))
    m_poses, m_rep, tol, rtol = bound(dict(poses=poses), fn)
    dp, dr = float(np.abs(host(out) - m_poses).max()), float(np.abs(host(rep) - m_rep).max())
    print(f"   |pose - model| {dp:.2e} (bound {tol:.2e}), |report - model| {dr:.2e} (bound {rtol:.2e})")
    assert dp <= tol and dr <= rtol and host(rep)[-1] == m_rep[-1] == 13
    # the heavy closure wins: its residual is the smaller one
    P = pg.as34(host(out))
    rel = pg.mul(P[2], pg.inv(P[8])).reshape(12)
    assert np.abs(rel - Z).max() < np.abs(rel - bad).max()
    g.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the drive
DRIVE = dict(outer=5, inner=64, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
INFO = dict(max_corr=1.0, min_inliers=10, min_ratio=1e-4, sigma_min=0.05, w_max=1e9)


def run_drive(drive, captured):
    """test_gpu_posegraph.run_drive with verify -> pairs_torch -> add_weighted -> gate -> relax behind the map append: eagerly, or as ONE
    graph captured behind the first eager step.  Returns per pose the host copies of what the step left, and the two logs at the end."""
    P = len(drive["pid"])
    res = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        lib = ctx.lib
        p = lambda t: t.data_ptr()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        pose, x, it, n, kid = z(12, torch.float64), z((60, 3), torch.float64), z(60, torch.float32), z(1, torch.int32), z(1, torch.int32)
        sig = z((1, 2400), torch.float64)
        mout = (z((1, STEP_K), torch.int32), z((1, STEP_K), torch.float64))
        oinfo, minfo, ginfo, gate_info = (z(4, torch.int32) for _ in range(4))
        win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
        km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
        odb = api.OnlineDatabase(ctx, "sc", KCAP, max_k=STEP_K)
        log, gated = api.PoseGraph(ctx, KCAP, 2 * KCAP), api.PoseGraph(ctx, KCAP, 2 * KCAP)
        gate = api.ClosureGate(ctx, log, gated, max_gap=20, min_support=1, rounds=4)
        ri = api.RegistrationInfo(ctx, STEP_K, MAXC)
        gate_out = dict(keep=z(2 * KCAP, torch.uint8), support=z(2 * KCAP, torch.int32), map=z(2 * KCAP, torch.int32), info=gate_info)
        corrected, report = z((KCAP, 12), torch.float64), z(DRIVE["outer"] + 2, torch.float64)
        out = win.empty_out()
        keep = dict(al=None, v=None, info=None)

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
            keep["v"] = km.verify_variants("sc", mout[0], keep["al"][0], (out["xyz"], out["offs"]), out["frame"][None], MAXC, hypotheses=2,
                                           max_corr=1.0, min_fitness=0.5, max_rmse=0.5, max_iter=10, out=keep["v"])
            keep["info"] = ri.pairs_torch((out["xyz"], out["offs"]), km, mout[0], keep["v"][0], keep["v"][2], MAXC, MAXC, out=keep["info"], **INFO)
            log.add_weighted_torch(mout[0], keep["v"][0], keep["info"].ok, minfo[1:2], keep["info"].w, info=ginfo)
            gate.run_map(km, **gate_out)
            gated.relax_map(km, out=corrected, report=report, **DRIVE)

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
            res.append(dict(idx=host(mout[0]), T=host(T), accepted=host(acc), map_info=host(minfo), log_info=host(ginfo), gate_info=host(gate_info),
                            corrected=host(corrected), report=host(report), **{k: host(t) for k, t in zip(FIELDS, keep["info"])}))
        logs = tuple({nm: host(getattr(q, nm)).copy() for nm in api.PoseGraph.NAMES} for q in (log, gated))
        del g
        ri.close(); gate.close(); gated.close(); log.close(); odb.close(); km.close(); win.close(); ctx.close()
    return res, logs


def test_one_captured_graph_from_verify_to_relax_equals_the_eager_calls(seq07):
    got, glogs = run_drive(seq07, captured=True)
    want, wlogs = run_drive(seq07, captured=False)
    model = pg.PoseGraphModel(2 * KCAP)
    logged = 0
    for i, (a, b) in enumerate(zip(got, want)):
        for k in a:
            assert same_bytes(a[k], b[k]), (i, k)
        # every logged edge carries its slot's w: the log is the restatement's filter of the step's own (idx, T, ok, w)
        info = rn.add_weighted(model, a["idx"], a["T"], a["ok"], int(a["map_info"][1]), a["w"])
        assert a["log_info"].tolist() == info.tolist(), (i, a["log_info"], info)
        assert not (a["ok"] & ~a["accepted"]).any()                 # a slot verify refused is OFF
        assert ((a["w"] > 0).all(axis=-1) == a["ok"].reshape(-1)).all()
        logged += int(info[0])
    for glog, wlog in zip(glogs, wlogs):
        for nm in api.PoseGraph.NAMES:
            assert same_bytes(glog[nm], wlog[nm]), nm
    for nm in api.PoseGraph.NAMES:
        assert same_bytes(glogs[0][nm], getattr(model, nm)), nm
    w = glogs[0]["edge_w"][:logged]
    print(f"   the drive: {logged} closures logged, w_rot {w[:, 0].min():.3g} .. {w[:, 0].max():.3g}, w_trans {w[:, 1].min():.3g} .. {w[:, 1].max():.3g}, "
          f"gate kept {int(got[-1]['gate_info'][1])}")
    assert logged >= 1 and (logged == 1 or len(np.unique(w, axis=0)) > 1)      # the weights differ from closure to closure
