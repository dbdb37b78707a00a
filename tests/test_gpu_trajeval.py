"""The trajectory evaluation on the device (pr_trajeval, trajeval.hip) against the NumPy restatement (trajeval_np.py).

Bit for bit: the whole ate block (counts, flags, argmax, S, the singular values - the Jacobi is restated rotation by rotation), err, the
centres, both prefixes, seg_end, every count, and every statistic made of + x / sqrt only (the d columns of rpe, mean c_rot, t_err and
the path ratio of seg, the d columns of clo and edge_err).
theta and what is summed from it (columns 4 .. 6 of rpe, r_err of seg, column 0 of edge_err, columns 2 .. 3 of clo): bounded by
trajeval_np.theta_tol - 100 x the difference between the restatement and a 50-digit evaluation of the same thetas, floored at 100
roundings of the largest theta, taken when the test runs and never from the device; r_err = theta / len takes the bound over the shortest
length.  A statistic of values that each move by at most tol moves by at most tol.
Guard words stand behind every output.  Nothing here provokes a fault: every out-of-range count or index is a clamp or a skip in the rule,
and the tests check the skip."""
import os
import subprocess

import numpy as np
import pytest
import torch

import posegraph_np as pg
import trajeval_np as tn
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd import eval as ev
from so_dso_place_recognition_amd.matcher import _stream_context

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ07 = os.path.join(ROOT, "tests", "golden", "ref_sequences", "kitti_seq07")
GUARD = -7.0
PAD = 5
NAMES = api.TrajEval._fields


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Rig:
    """a handle, its inputs on the device and guarded outputs: every array PAD elements longer than stated, the excess and - before
    each run - the array itself filled with the guard pattern"""

    def __init__(self, est, gt, valid=None, log=None, ctx=None, **kw):
        self.own = ctx is None
        self.ctx = ctx or _stream_context(0)
        est = np.asarray(est)
        est = est[None] if est.ndim == 2 else est
        self.kw = kw
        self.te = api.TrajectoryEval(self.ctx, est.shape[1], B=est.shape[0], **kw)
        self.est_np, self.gt_np, self.valid_np = est, np.asarray(gt), valid
        self.est, self.gt = dev(est), dev(gt)
        self.valid = None if valid is None else dev(valid, np.uint8)
        self.nd = torch.full((4,), int(GUARD), dtype=torch.int32, device="cuda")
        self.log = log
        self.big = {}
        for name, (shape, dt) in self.te.shapes(log is not None).items():
            self.big[name] = torch.empty(int(np.prod(shape)) + PAD, dtype=torch.int32 if dt == np.int32 else torch.float64, device="cuda")
        self.out = {name: self.big[name][:self.big[name].numel() - PAD] for name in self.big}

    def run(self, n):
        self.nd[0] = n
        for t in self.big.values():
            t.fill_(GUARD)
        self.te.run_torch(self.est, self.nd, self.gt, valid=self.valid, log=self.log, out=self.out, optional=())
        self.ctx.sync()
        return self.read()

    def read(self):
        got = {}
        for name, (shape, dt) in self.te.shapes(self.log is not None).items():
            a = self.big[name].cpu().numpy()
            assert (a[-PAD:] == GUARD).all(), (name, "a guard word was written")
            got[name] = a[:-PAD].reshape(shape).copy()
        return got

    def want(self, n, log=None):
        kw = dict(self.kw)
        kw.pop("rot_thr", None), kw.pop("trans_thr", None)
        ec = kw.pop("edge_capacity", 0)
        return tn.evaluate(self.est_np, n, self.gt_np, valid=self.valid_np, log=log, edge_capacity=ec, rot_thr=self.te.params.rot_thr,
                           trans_thr=self.te.params.trans_thr, **kw)

    def close(self):
        self.te.close()
        if self.own:
            self.ctx.close()


def check(got, want, what, lengths=()):
    """the contracts of the module's docstring; returns the theta bound used"""
    aux = want["aux"]
    for name in ("ate", "err", "centres", "prefix"):
        assert same_bytes(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:4])
    tol = 0.0
    if "rpe" in got:
        tol = tn.theta_tol(aux["rpe_E"], aux["rpe_theta"])
        g, w = got["rpe"], want["rpe"]
        assert same_bytes(g[..., [0, 1, 2, 3, 7]], w[..., [0, 1, 2, 3, 7]]), (what, "rpe", g, w)
        assert np.abs(g[..., 4:7] - w[..., 4:7]).max() <= tol, (what, "rpe theta", np.abs(g[..., 4:7] - w[..., 4:7]).max(), tol)
    if "seg" in got:
        stol = tn.theta_tol(aux["seg_E"], aux["seg_theta"]) / min(lengths)
        g, w = got["seg"], want["seg"]
        assert same_bytes(got["seg_end"], want["seg_end"]), (what, "seg_end")
        assert same_bytes(g[..., [0, 1, 3]], w[..., [0, 1, 3]]), (what, "seg", g, w)
        assert np.abs(g[..., 2] - w[..., 2]).max() <= stol, (what, "seg r_err", np.abs(g[..., 2] - w[..., 2]).max(), stol)
        tol = max(tol, stol)
    if "clo" in got:
        ctol = tn.theta_tol(aux["clo_E"], aux["clo_theta"])
        g, w = got["clo"], want["clo"]
        assert same_bytes(got["edge_err"][:, 1], want["edge_err"][:, 1]) and same_bytes(g[[0, 1, 4, 5, 6, 7]], w[[0, 1, 4, 5, 6, 7]]), (what, "clo", g, w)
        assert np.abs(got["edge_err"][:, 0] - want["edge_err"][:, 0]).max() <= ctol and np.abs(g[2:4] - w[2:4]).max() <= ctol, (what, "clo theta")
        tol = max(tol, ctol)
    return tol


# ------------------------------------------------------------------------------------------------ 1. sizes, rows, deltas, lengths
CAP = 300
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257]                 # the tree's and the prefix's chunk is 256: one step on either side of it


@pytest.mark.parametrize("n", SIZES)
def test_equals_the_restatement_over_row_counts(n):
    """B = 3, holes in valid, a NaN and an Inf row in est of the last b only and an Inf row in gt; deltas 1, 2, 7, n - 1, n, n + 5; lengths
    below one step, equal to a prefix value exactly, ordinary, and above the whole path; the rows behind n hold finite garbage"""
    est, gt, valid = tn.case(n, cap=CAP, B=3, seed=n, holes=True, bad=True)
    exact = float(tn.evaluate(est, n, gt, valid=valid, align="sim3")["prefix"][0, 0, min(10, max(n - 1, 0))]) or 3.0
    deltas, lengths = (1, 2, 7, max(n - 1, 1), max(n, 1), n + 5), (0.25, exact, 20.0, 1e6)
    rig = Rig(est, gt, valid, align="sim3", gt_kind="c2w", deltas=deltas, lengths=lengths, step=1)
    got, want = rig.run(n), rig.want(n)
    tol = check(got, want, n, lengths)
    a = want["ate"]
    print(f"   n {n}: used {a[:, 0].tolist()} flags {a[:, 19].tolist()} s {a[:, 6].tolist()} pairs {want['rpe'][0, :, 0].tolist()} "
          f"segments {want['seg'][0, :, 0].tolist()} theta bound {tol:.2e}")
    assert a[0, 0] == sum(1 for i in range(n) if valid[i] and not (n > 6 and i == 2)) and (n < 7 or a[2, 0] < a[0, 0])      # the bad est rows count for b = 2 only
    assert (want["rpe"][:, 4:, 0] == 0).all() and (want["seg"][:, 3, 0] == 0).all()      # delta n, n + 5 and the length above the path: nothing
    if n >= 64:
        e = want["seg_end"][0, 0]
        assert e[0] == 1 and e[1] > 10 and want["prefix"][0, 0, e[1] - 1] == exact      # strict: the row that meets the length does not end it
    rig.close()


@pytest.mark.parametrize("align,kind", [("none", "c2w"), ("first", "c2w"), ("first", "w2c"), ("se3", "w2c"), ("sim3", "w2c"), ("se3", "positions"),
                                        ("sim3", "positions"), ("none", "positions")])
def test_every_alignment_and_ground_truth_kind(align, kind):
    est, gt, valid = tn.case(257, cap=260, B=1, seed=3, gt_kind=kind, holes=True, bad=True)
    tables = dict(deltas=(), lengths=()) if kind == "positions" else dict(deltas=(1, 10), lengths=(30.0, 100.0))
    rig = Rig(est, gt, valid, align=align, gt_kind=kind, step=1, **tables)
    got, want = rig.run(257), rig.want(257)
    check(got, want, (align, kind), tables["lengths"])
    print(f"   {align} {kind}: ATE rmse {want['ate'][0, 2]:.4f} s {want['ate'][0, 6]:.5f} flags {want['ate'][0, 19]:.0f}")
    rig.close()


def test_standstill_stretch_and_step_10():
    est, gt, valid = tn.case(257, cap=257, B=1, seed=5, standstill=range(40, 61))
    rig = Rig(est, gt, valid, align="se3", gt_kind="c2w", deltas=(1, 7), lengths=(0.5, 15.0), step=10)
    got, want = rig.run(257), rig.want(257)
    check(got, want, "standstill", (0.5, 15.0))
    assert got["seg_end"].shape == (1, 26, 2) and got["seg_end"][0, 5, 0] == 61 and got["seg_end"][0, 4, 0] == 61      # rows 40 .. 60 stand still
    assert (got["prefix"][0, 0, 40:61] == got["prefix"][0, 0, 39]).all()
    rig.close()


def test_degenerate_alignments_on_the_device():
    t = np.linspace(0.0, 100.0, 70)
    x = np.outer(t, [0.6, 0.0, 0.8])
    est = np.zeros((2, 70, 12))
    est[:, :, [0, 5, 10]] = 1.0
    est[0, :, [3, 7, 11]] = -x.T                                    # b = 0: a straight road
    est[1, :, [3, 7, 11]] = np.array([[1.0], [2.0], [3.0]])          # b = 1: a standstill
    gt = x @ tn.rot([1.0, 1.0, 0.0], 0.7).T + [5e6, 200.0, -50.0]
    rig = Rig(est, gt, None, align="sim3", gt_kind="positions", deltas=(), lengths=())
    got, want = rig.run(70), rig.want(70)
    check(got, want, "degenerate")
    assert got["ate"][:, 19].tolist() == [tn.DEGENERATE, tn.DEGENERATE | tn.NO_SCALE] and got["ate"][0, 2] < 1e-7
    got, want = rig.run(2), rig.want(2)
    check(got, want, "few")
    assert got["ate"][:, 19].tolist() == [tn.FEW, tn.FEW] and (got["ate"][:, 6] == 1.0).all()
    rig.close()


@pytest.mark.parametrize("scribble", [1 << 30, -3])
def test_a_scribbled_count_is_clamped_before_it_forms_an_address(scribble):
    est, gt, valid = tn.case(65, cap=65, B=1, seed=9)
    rig = Rig(est, gt, valid, align="se3", gt_kind="c2w", deltas=(1, 64), lengths=(10.0,), step=1)
    got = rig.run(scribble)
    check(got, rig.want(scribble), scribble, (10.0,))
    assert got["ate"][0, 0] == (65 if scribble > 0 else 0)
    rig.close()


# ------------------------------------------------------------------------------------------------ 2. closures
def closure_log(ctx, W, pairs, Z, count, cap):
    g = api.PoseGraph(ctx, len(W), cap)
    eij = np.zeros((cap, 2), np.int32)
    eij[:len(pairs)] = pairs
    ez = np.zeros((cap, 12))
    ez[:len(Z)] = Z
    g.edge_ij.copy_(dev(eij, np.int32)); g.edge_Z.copy_(dev(ez)); g.state.copy_(dev([count, 0, 0, 0], np.int32))
    return g, (eij, ez, np.array([count, 0, 0, 0]))


def true_Z(W, i, j):
    R, t = tn.split(W)
    Rz, tz = tn.rigid_mul(R[i], t[i], *tn.rigid_inv(R[j], t[j]))
    return np.hstack([Rz, tz[:, None]]).reshape(-1)


def test_invalid_edges_are_skipped_and_thresholds_are_strict():
    """the kinds of invalid edge of the gate's validity case - i = -1, j = n, i == j, a NaN in Z, a row whose gt is not finite - and a row
    that is not valid, an edge behind the count; then trans_thr met exactly and one ulp below the edge's d"""
    n, cap = 50, 52
    G = tn.drive(cap, 4)
    W = tn.invert_rows(G)
    pairs = [(3, 40), (10, 45), (5, 5), (-1, 7), (7, n), (8, 20), (2, 30), (12, 33), (6, 41), (9, 44)]
    Z = np.array([true_Z(W, min(max(i, 0), cap - 1), min(max(j, 0), cap - 1)) for i, j in pairs])
    Z[1, 3] += 0.5
    Z[7, 7] -= 0.125
    Z[5, 7] = np.nan
    gt = G.copy()
    gt[30, 2] = np.inf
    valid = np.ones(cap, np.uint8)
    valid[41] = 0
    ctx = _stream_context(0)
    g, log = closure_log(ctx, W, pairs, Z, 9, 12)                  # the tenth edge lies behind the count
    base = dict(align="none", gt_kind="c2w", deltas=(), lengths=(), edge_capacity=12, rot_thr=10.0)
    d1 = float(tn.evaluate(W, n, gt, valid=valid, log=log, edge_capacity=12)["edge_err"][1, 1])
    wrongs = []
    for thr in (d1, float(np.nextafter(d1, 0.0)), 0.1):
        rig = Rig(W, gt, valid, log=g, ctx=ctx, trans_thr=thr, **base)
        got, want = rig.run(n), rig.want(n, log)
        check(got, want, thr)
        assert (got["edge_err"][[2, 3, 4, 5, 6, 8, 9, 10, 11]] == -1).all() and (got["edge_err"][[0, 1, 7]] >= 0).all()
        assert got["clo"][0] == 3 and got["clo"][6] == 9 and got["edge_err"][1, 1] == d1
        wrongs.append(int(got["clo"][1]))
        rig.close()
    assert wrongs == [0, 1, 2]                                      # d == thr is not wrong; d one ulp above thr is; at 0.1 edge 7 (0.125 m) is too
    g.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. forms
def test_host_form_two_runs_and_one_capture_for_every_count():
    cap, EC = 300, 8
    est, gt, valid = tn.case(cap, cap=cap, B=2, seed=21, holes=True)
    W = tn.invert_rows(tn.drive(cap, 21))
    pairs = [(4, 40), (11, 250), (60, 200), (5, 291)]
    Z = np.array([true_Z(W, i, j) for i, j in pairs])
    Z[:, 3] += [0.0, 0.25, 0.5, 0.75]
    kw = dict(align="sim3", gt_kind="c2w", deltas=(1, 10), lengths=(10.0, 50.0), step=3, edge_capacity=EC, rot_thr=0.01, trans_thr=0.3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        g, log = closure_log(ctx, W, pairs, Z, 0, EC)
        rig = Rig(est, gt, valid, log=g, ctx=ctx, **kw)
        rig.run(0)                                                  # one eager call, then the capture of the same call at n = 0, no edge
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            rig.te.run_torch(rig.est, rig.nd, rig.gt, valid=rig.valid, log=g, out=rig.out, optional=())
        for n, edges in ((40, 1), (300, 4), (257, 3)):              # three node and edge counts under the one capture
            rig.nd[0] = n
            g.state[0] = edges
            log = (log[0], log[1], np.array([edges, 0, 0, 0]))
            for t in rig.big.values():
                t.fill_(GUARD)
            graph.replay()
            st.synchronize()
            replay = rig.read()
            eager, again = rig.run(n), rig.run(n)
            host = rig.te.run(rig.est, rig.nd, rig.gt, valid=rig.valid, log=g)
            want = rig.want(n, log)
            check(eager, want, (n, edges), kw["lengths"])
            for name in replay:
                assert same_bytes(replay[name], eager[name]) and same_bytes(eager[name], again[name]), (n, name)
                assert same_bytes(np.asarray(getattr(host, name)), eager[name]), (n, name, "host form")
            assert eager["clo"][0] == sum(1 for i, j in pairs[:edges] if i < n and j < n and valid[i] and valid[j]) and eager["clo"][6] == edges
        del graph
        rig.close(); g.close(); ctx.close()


def test_host_form_without_optional_outputs():
    """pr_trajeval_run with none and with some of err, seg_end, centres, prefix: every output that was passed equals, byte for byte, that of
    the call with all of them, at the file's smallest rig"""
    est, gt, valid = tn.case(65, cap=65, B=1, seed=9)
    rig = Rig(est, gt, valid, align="se3", gt_kind="c2w", deltas=(1, 64), lengths=(10.0,), step=1)
    rig.nd[0] = 65
    full = rig.te.run(rig.est, rig.nd, rig.gt, valid=rig.valid)
    assert all(getattr(full, name) is not None for name in ("ate", "rpe", "seg", "err", "seg_end", "centres", "prefix"))
    for optional in ((), ("err", "prefix"), ("seg_end", "centres")):
        part = rig.te.run(rig.est, rig.nd, rig.gt, valid=rig.valid, optional=optional)
        for name in rig.te.NAMES:
            if getattr(full, name) is not None and (name in ("ate", "rpe", "seg") or name in optional):
                assert same_bytes(getattr(part, name), getattr(full, name)), (optional, name)
            else:
                assert getattr(part, name) is None, (optional, name)
    rig.close()


def test_relax_then_evaluate_as_one_graph_on_the_two_lap_circle():
    """test_gpu_posegraph.py's consistent graph: the relaxation recovers ground truth there, so the ATE after it is below the ATE before"""
    c = pg.consistent_case()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, 12, 1024, 64)
        g = api.PoseGraph(ctx, 12, 32, max_outer=6, max_inner=72)
        for (i, j), Z in zip(c["pairs"], c["Z"]):
            g.add([i], Z, [1], j)
        km.poses.copy_(dev(c["poses"]))
        km.state[0] = 12
        gt = dev(c["gt"])
        te = api.TrajectoryEval(ctx, 12, align="none", gt_kind="w2c", deltas=(1,), lengths=(5.0,), step=1)
        relaxed = torch.zeros((12, 12), dtype=torch.float64, device="cuda")
        report = torch.zeros(8, dtype=torch.float64, device="cuda")
        outs = [{n: torch.zeros(s, dtype=torch.int32 if dt == np.int32 else torch.float64, device="cuda") for n, (s, dt) in te.shapes(False).items()}
                for _ in range(2)]

        def step(out):
            g.relax_map(km, out=relaxed, report=report, **c["params"])
            return te.run_map(km, gt, poses=relaxed, out=out, optional=())

        before = te.run_map(km, gt)
        eager = step(outs[0])
        st.synchronize()
        eager = {n: getattr(eager, n).cpu().numpy().copy() for n in outs[0]}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            step(outs[1])
        relaxed.zero_()
        graph.replay()
        st.synchronize()
        for n in outs[1]:
            assert same_bytes(outs[1][n].cpu().numpy(), eager[n]), n
        check(eager, tn.evaluate(relaxed.cpu().numpy(), 12, c["gt"], align="none", gt_kind="w2c", deltas=(1,), lengths=(5.0,)), "circle", (5.0,))
        b, a = float(before.ate[0, 2]), float(eager["ate"][0, 2])
        print(f"   two-lap circle: ATE rmse before {b:.3e}, after the relaxation {a:.3e}")
        assert a < b and b > 1e-3
        del graph
        te.close(); g.close(); km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the committed sequence and the executable
@pytest.fixture(scope="module")
def seq07_rows():
    ids, poses = ev.load_pose_history(SEQ07)
    inc = np.loadtxt(os.path.join(SEQ07, "incoming_id_file.txt")).astype(np.int64)
    return poses[np.isin(ids, inc)], ev.load_kitti_gt_poses(SEQ07)


def test_seq07_equals_the_restatement_and_the_executable_prints_the_same_numbers(seq07_rows, tmp_path):
    est, gt = seq07_rows
    n = len(est)
    lengths = tuple(100.0 * k for k in range(1, 9))
    rig = Rig(est, gt, None, align="sim3", gt_kind="c2w", deltas=(1, 10), lengths=lengths, step=1)
    got, want = rig.run(n), rig.want(n)
    check(got, want, "seq07", lengths)
    a = got["ate"][0]
    print(f"   seq07: N {a[0]:.0f} ATE rmse {a[2]:.4f} s {a[6]:.5f}; RPE(1) {got['rpe'][0, 0, 1]:.4f} m; segments {got['seg'][0, 8].tolist()}")
    rig.close()
    np.savetxt(tmp_path / "poses.txt", np.hstack([np.arange(n)[:, None], est]), fmt="%.17g")
    np.savetxt(tmp_path / "gt.txt", gt, fmt="%.17g")
    exe = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin", "eval_trajectory")
    r = subprocess.run([exe, f"_poses:={tmp_path / 'poses.txt'}", f"_gt:={tmp_path / 'gt.txt'}", "_gt_kind:=c2w", "_align:=sim3"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 + 2 + 9
    num = lambda line, key: float(line.split()[line.split().index(key) + 1])
    assert num(lines[0], "used") == a[0] and num(lines[1], "rmse") == a[2] and num(lines[1], "max") == a[4] and num(lines[2], "s") == a[6]
    for k in range(2):
        assert num(lines[3 + k], "pairs") == got["rpe"][0, k, 0] and num(lines[3 + k], "trans_rmse") == got["rpe"][0, k, 1]
        assert num(lines[3 + k], "rot_mean") == got["rpe"][0, k, 5]
    for l in range(9):
        assert num(lines[5 + l], "segments") == got["seg"][0, l, 0] and num(lines[5 + l], "t_err") == got["seg"][0, l, 1]
        assert num(lines[5 + l], "r_err") == got["seg"][0, l, 2] and num(lines[5 + l], "ratio") == got["seg"][0, l, 3]


def test_refusals_on_a_live_handle():
    ctx = _stream_context(0)
    te = api.TrajectoryEval(ctx, 16, deltas=(1,), lengths=(5.0,))
    est, gt = torch.zeros((1, 16, 12), dtype=torch.float64, device="cuda"), torch.zeros((16, 12), dtype=torch.float64, device="cuda")
    n = torch.zeros(4, dtype=torch.int32, device="cuda")
    g = api.PoseGraph(ctx, 16, 4)
    with pytest.raises(ValueError, match="edge_capacity"):
        te.run_torch(est, n, gt, log=g)
    with pytest.raises(ValueError, match="est"):
        te.run_torch(est[:, :8], n, gt)
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    o = _lib.TrajEvalOut()
    assert te.lib.pr_trajeval_run_dev(te.h, p(est), p(n), p(gt), None, None, C.byref(o)) == _lib.PR_EINVAL
    assert "out.ate is NULL" in te.lib.pr_last_error(ctx.h).decode()
    assert te.lib.pr_trajeval_run_dev(te.h, None, p(n), p(gt), None, None, C.byref(o)) == _lib.PR_EINVAL
    rec = _lib.PoseGraphBuffers(*(C.c_void_p(getattr(g, nm).data_ptr()) for nm in g.NAMES))
    ate = torch.zeros(24, dtype=torch.float64, device="cuda")
    o.ate, o.rpe, o.seg = ate.data_ptr(), ate.data_ptr(), ate.data_ptr()
    assert te.lib.pr_trajeval_run_dev(te.h, p(est), p(n), p(gt), None, C.byref(rec), C.byref(o)) == _lib.PR_EINVAL
    assert "edge_capacity is 0" in te.lib.pr_last_error(ctx.h).decode()
    assert te.scratch_bytes() > 0
    g.close(); te.close(); ctx.close()
