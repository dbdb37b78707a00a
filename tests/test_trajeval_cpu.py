"""The trajectory evaluation without a device (pr_trajeval): the header's rule text, the exported and bound symbols, the
scratch formula, every refusal that comes before a device is touched, and the NumPy restatement (trajeval_np.py) against references that
share none of its arithmetic - the extended-precision Kabsch of icp_mp.py and an mpmath Umeyama scale for the alignment, math.fsum for
the prefixes, a linear scan for the segment search - and on the committed seq06 / seq07 fixtures.

Alignment bounds (derived, not measured).  The covariance is a sum of N <= 200 products and carries a relative rounding of about N eps;
a rotation taken from it moves by that perturbation over the gap sigma_2 + d sigma_3 (Kabsch's conditioning), and ten Jacobi sweeps add a
few eps each: |R - R_mp| <= 1000 eps sigma_1 / (sigma_2 + d sigma_3).  t = my - s R mx inherits that times |mx| plus the rounding of
numbers of size |mx| + |my|; s is a ratio of two such sums: 1000 eps relative.
Prefix bound: every dist[i] is reached through at most C + 256 additions of non-negative terms (C inside the block, 255 block totals, 1 for
base + w), so |dist[i] - exact| <= (C + 257) eps dist[i]."""
import ctypes as C
import math
import os
import re
import subprocess

import mpmath
import numpy as np
import pytest

import icp_mp
import trajeval_np as tn
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd import eval as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = os.path.join(ROOT, "tests", "golden", "ref_sequences")
EPS = tn.EPS
NAMES = ("pr_trajeval_create", "pr_trajeval_run_dev", "pr_trajeval_run", "pr_trajeval_scratch_bytes", "pr_trajeval_destroy")


def header():
    return open(os.path.join(ROOT, "include", "place_recognition.h")).read()


# ------------------------------------------------------------------------------------------------ 1. header, symbols, formula, refusals
def test_header_carries_the_rule_and_the_symbols_are_bound():
    h = header()
    for phrase in ("THE TREE", "Umeyama", "PR_TRAJ_DEGENERATE iff", "dist[j] > dist[f] + len", "rel_gt^-1 rel_est", "atan2(|v|, 0.5 (tr - 1))",
                   "tests/trajeval_np.py", "a route at a UTM northing", "BLOCKED order", "PR_TRAJ_GT_POSITIONS"):
        assert phrase in h, phrase
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    for name, val in (("ALIGN_NONE", 0), ("ALIGN_FIRST", 1), ("ALIGN_SE3", 2), ("ALIGN_SIM3", 3), ("GT_W2C", 0), ("GT_C2W", 1), ("GT_POSITIONS", 2),
                      ("FEW", 1), ("DEGENERATE", 2), ("NO_SCALE", 4), ("ATE_STATS", 24), ("RPE_STATS", 8), ("SEG_STATS", 4), ("CLO_STATS", 8)):
        assert re.search(rf"#define PR_TRAJ_{name} {val}\b", h) and getattr(_lib, "TRAJ_" + name) == val, name
    assert C.sizeof(_lib.TrajEvalParams) == 48 and C.sizeof(_lib.TrajEvalOut) == 72
    assert (tn.FEW, tn.DEGENERATE, tn.NO_SCALE) == (_lib.TRAJ_FEW, _lib.TRAJ_DEGENERATE, _lib.TRAJ_NO_SCALE)


def params(**kw):
    d = dict(node_capacity=100, batch=2, align=3, gt_kind=1, n_deltas=2, n_lengths=3, step=4, edge_capacity=10, rot_thr=0.1, trans_thr=1.0)
    d.update(kw)
    return _lib.TrajEvalParams(*(d[n] for n, _ in _lib.TrajEvalParams._fields_))


def r16(x):
    return (x + 15) & ~15


@pytest.mark.parametrize("cap,B,K,L,step,EC", [(100, 2, 2, 3, 4, 10), (1, 1, 0, 0, 1, 0), (4097, 64, 8, 8, 10, 65536), (1 << 20, 1, 1, 1, 1, 0)])
def test_scratch_formula(cap, B, K, L, step, EC):
    lib = _lib.load()
    slots = -(-cap // step)
    want = sum(r16(x) for x in (4 * B * cap, 4 * cap, 24 * (B + 1) * cap, 16 * B * cap, 128 * B, 32 * B * L, 32, 64, 192 * B, 64 * B * K, 32 * B * (L + 1), 64,
                                8 * B * cap, 4 * B * slots * L, 16 * EC))
    p = params(node_capacity=cap, batch=B, n_deltas=K, n_lengths=L, step=step, edge_capacity=EC)
    assert lib.pr_trajeval_scratch_bytes(C.byref(p)) == want
    assert lib.pr_trajeval_scratch_bytes(None) == 0


REFUSED = [
    (dict(node_capacity=0), "node_capacity"), (dict(node_capacity=(1 << 20) + 1), "node_capacity"), (dict(batch=0), "batch"), (dict(batch=65), "batch"),
    (dict(align=4), "align"), (dict(align=-1), "align"), (dict(gt_kind=3), "gt_kind"), (dict(n_deltas=9), "n_deltas"), (dict(n_deltas=-1), "n_deltas"),
    (dict(n_lengths=9), "n_lengths"), (dict(step=0), "step"), (dict(edge_capacity=-1), "edge_capacity"), (dict(edge_capacity=65537), "edge_capacity"),
    (dict(gt_kind=2), "positions"), (dict(gt_kind=2, n_deltas=0, n_lengths=0), "positions"),
    (dict(gt_kind=2, n_deltas=0, n_lengths=0, edge_capacity=0, align=1), "positions"), (dict(rot_thr=float("nan")), "rot_thr"),
    (dict(trans_thr=-1.0), "trans_thr"),
]


@pytest.mark.parametrize("kw,word", REFUSED)
def test_bad_sizes_are_refused_before_a_device_is_touched(kw, word):
    lib = _lib.load()
    p = params(**kw)
    h = C.c_void_p(5)
    deltas, lengths = (C.c_int32 * 8)(*[1] * 8), (C.c_double * 8)(*[10.0] * 8)
    assert lib.pr_trajeval_create(None, C.byref(p), deltas, lengths, C.byref(h)) == _lib.PR_EINVAL and not h
    assert word in lib.pr_last_error(None).decode()
    assert lib.pr_trajeval_scratch_bytes(C.byref(p)) == 0


def test_bad_tables_and_null_pointers_are_refused_before_a_device_is_touched():
    lib = _lib.load()
    p = params()
    h = C.c_void_p()
    good_d, good_l = (C.c_int32 * 8)(*[1] * 8), (C.c_double * 8)(*[10.0] * 8)

    def refused(deltas, lengths, word, pp=p, out=h):
        assert lib.pr_trajeval_create(None, C.byref(pp) if pp is not None else None, deltas, lengths, C.byref(out) if out is not None else None) == _lib.PR_EINVAL
        assert word in lib.pr_last_error(None).decode(), lib.pr_last_error(None)

    refused(good_d, good_l, "out is NULL", out=None)
    refused(good_d, good_l, "params is NULL", pp=None)
    refused(None, good_l, "table is NULL")
    refused(good_d, None, "table is NULL")
    refused((C.c_int32 * 8)(1, 0), good_l, "deltas[1]")
    for bad in (0.0, -5.0, float("inf"), float("nan")):
        refused(good_d, (C.c_double * 8)(10.0, 20.0, bad), "lengths[2]")
    refused(good_d, good_l, "ctx is NULL")                         # everything else is in order: only now the context is looked at
    for fn in (lib.pr_trajeval_run_dev, lib.pr_trajeval_run):
        assert fn(None, None, None, None, None, None, None) == _lib.PR_EINVAL and "handle is NULL" in lib.pr_last_error(None).decode()
    lib.pr_trajeval_destroy(None)
    with pytest.raises(ValueError, match="align"):
        api.TrajectoryEval(None, 10, align="affine")
    with pytest.raises(ValueError, match="gt_kind"):
        api.TrajectoryEval(None, 10, gt_kind="utm")


def test_the_executable_prints_the_librarys_refusal(tmp_path):
    exe = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin", "eval_trajectory")
    rows = tn.drive(5, 1)
    np.savetxt(tmp_path / "p.txt", tn.invert_rows(rows))
    np.savetxt(tmp_path / "g.txt", rows)
    r = subprocess.run([exe, f"_poses:={tmp_path / 'p.txt'}", f"_gt:={tmp_path / 'g.txt'}", "_align:=affine"], capture_output=True, text=True)
    assert r.returncode == 2 and "pr_trajeval_create: align=-1 is no mode" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([exe, f"_poses:={tmp_path / 'p.txt'}", f"_gt:={tmp_path / 'g.txt'}", "_step:=0"], capture_output=True, text=True)
    assert r.returncode == 2 and "step=0" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([exe, f"_poses:={tmp_path / 'p.txt'}"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr


# ------------------------------------------------------------------------------------------------ 2. the alignment against mpmath
def poses_at(x):
    """W2C rows [I | -x]: their camera centres are exactly x"""
    x = np.asarray(x, np.float64)
    p = np.zeros((len(x), 12))
    p[:, [0, 5, 10]] = 1.0
    p[:, [3, 7, 11]] = -x
    return p


def align_np(x, y, mode, n=None):
    n = len(x) if n is None else n
    o = tn.evaluate(poses_at(x), n, y, align=mode, gt_kind="positions")
    a = o["ate"][0]
    assert np.array_equal(o["centres"][0][:n], x[:n]) and np.array_equal(o["centres"][1][:n], y[:n]) and not o["centres"][:, n:].any()
    return dict(N=a[0], rmse=a[2], s=a[6], R=a[7:16].reshape(3, 3), t=a[16:19], flags=int(a[19]), sig=a[20:23], varx=a[23], err=o["err"][0])


def umeyama_mp(x, y):
    """(R, t, s_sim3, t_sim3, sigma, d) in 60 digits: icp_mp's Kabsch for the rotation, the scale tr(D Sigma) / sum |x - mx|^2 beside it"""
    k = icp_mp.kabsch_update(x, y, np.hstack([np.eye(3), np.zeros((3, 1))]))
    with mpmath.workdps(60):
        X = [[mpmath.mpf(float(v)) for v in r] for r in x]
        Y = [[mpmath.mpf(float(v)) for v in r] for r in y]
        n = len(X)
        mx = [sum(r[c] for r in X) / n for c in range(3)]
        my = [sum(r[c] for r in Y) / n for c in range(3)]
        sx = sum((r[c] - mx[c]) ** 2 for r in X for c in range(3))
        s = (mpmath.mpf(k["s"][0]) + mpmath.mpf(k["s"][1]) + k["d"] * mpmath.mpf(k["s"][2])) / sx if sx > 0 else mpmath.mpf(1)
        R = k["T"][:, :3]
        Rm = mpmath.matrix([[mpmath.mpf(float(v)) for v in r] for r in R])
        t = [float(my[a] - s * sum(Rm[a, c] * mx[c] for c in range(3))) for a in range(3)]
    return dict(R=R, t_se3=k["T"][:, 3], s=float(s), t_sim3=np.array(t), sig=k["s"], d=k["d"], mx=k["mu_p"], my=k["mu_q"])


def check_alignment(x, y, what):
    ref = umeyama_mp(x, y)
    s1, s2, s3 = ref["sig"]
    tol_R = 1000 * EPS * s1 / (s2 + ref["d"] * s3)
    size = float(np.abs(ref["mx"]).max() + np.abs(ref["my"]).max())
    for mode in ("se3", "sim3"):
        got = align_np(x, y, mode)
        s_ref, t_ref = (1.0, ref["t_se3"]) if mode == "se3" else (ref["s"], ref["t_sim3"])
        dR, dt, ds = np.abs(got["R"] - ref["R"]).max(), np.abs(got["t"] - t_ref).max(), abs(got["s"] - s_ref)
        print(f"   {what} {mode}: |R - mp| {dR:.2e} (bound {tol_R:.2e}) |t - mp| {dt:.2e} (bound {(3 * tol_R + 1000 * EPS) * size:.2e}) "
              f"|s - mp| {ds:.2e} rmse {got['rmse']:.3e} d {ref['d']}")
        assert got["flags"] == 0 and got["N"] == len(x)
        assert dR <= tol_R and dt <= (3 * tol_R + 1000 * EPS) * size and ds <= 1000 * EPS * s_ref
        assert abs(np.linalg.det(got["R"]) - 1.0) < 1e-13
    return ref


def test_planted_similarity_at_a_utm_offset():
    rng = np.random.default_rng(7)
    x = rng.normal(size=(200, 3)) * [100.0, 60.0, 5.0]
    R = tn.rot(rng.normal(size=3), 2.1)
    y = 0.97 * x @ R.T + np.array([5.0e6, -3.2e6, 140.0]) + 0.01 * rng.normal(size=(200, 3))
    ref = check_alignment(x, y, "planted")
    assert abs(ref["s"] - 0.97) < 1e-3 and np.abs(ref["R"] - R).max() < 1e-3
    got = align_np(x, y, "sim3")
    assert got["rmse"] < 0.03                                       # the centred second pass: nothing of the 5e6 is left in the residual


def test_planar_set_with_a_negative_determinant_takes_the_reflection_correction():
    rng = np.random.default_rng(8)
    a = rng.normal(size=(150, 3)) * [40.0, 25.0, 1e-6]
    R = tn.rot([0.3, -1.0, 0.2], 1.3)
    mirrored = a * [1.0, 1.0, -1.0]                                 # the off-plane part mirrored: det of the covariance < 0
    y = mirrored @ R.T + [10.0, 20.0, 30.0]
    ref = check_alignment(a, y, "planar")
    assert ref["d"] == -1
    got = align_np(a, y, "se3")
    assert np.abs(got["R"] - R).max() < 1e-6                        # a rotation, not the mirror image


def test_straight_line_and_standstill_are_flagged_and_still_return_a_rigid_map():
    t = np.linspace(0.0, 300.0, 120)
    x = np.outer(t, [0.6, 0.0, 0.8])
    R = tn.rot([1.0, 1.0, 0.0], 0.7)
    y = x @ R.T + [100.0, 200.0, -50.0]
    for mode in ("se3", "sim3"):
        got = align_np(x, y, mode)
        assert got["flags"] == tn.DEGENERATE
        assert np.abs(got["R"] @ got["R"].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(got["R"]) - 1.0) < 1e-14
        assert got["rmse"] < 1e-10 and abs(got["s"] - 1.0) < 1e-12  # the line is taken onto the line
    p = np.tile([[3.0, -4.0, 12.0]], (50, 1))
    got = align_np(p, p + [1.0, 2.0, 3.0], "sim3")
    assert got["flags"] == tn.DEGENERATE | tn.NO_SCALE and got["s"] == 1.0 and np.array_equal(got["R"], np.eye(3))
    assert np.array_equal(got["t"], [1.0, 2.0, 3.0]) and got["rmse"] == 0.0
    got = align_np(x, y, "sim3", n=2)                               # two rows: too few, the identity
    assert got["flags"] == tn.FEW and got["N"] == 2 and got["s"] == 1.0 and np.array_equal(got["R"], np.eye(3)) and not got["t"].any()
    got = align_np(x, y, "se3", n=0)
    assert got["flags"] == tn.FEW and got["N"] == 0 and got["rmse"] == 0.0


def test_first_and_none_modes():
    G = tn.drive(30, 3)
    est = tn.invert_rows(G)
    o = tn.evaluate(est, 30, G, align="none", gt_kind="c2w")
    assert o["ate"][0][2] < 1e-13 and o["ate"][0][6] == 1.0
    Rw, tw = tn.rot([1, 2, 3], 0.8), np.array([4.0, 5.0, 6.0])
    moved = tn.perturb(G, 0, noise=0.0, rigid=(Rw, tw))            # the est world is a rigid copy of the gt world
    for kind, gt in (("c2w", G), ("w2c", tn.invert_rows(G))):
        o = tn.evaluate(moved, 30, gt, align="first", gt_kind=kind)
        assert o["ate"][0][2] < 1e-12 and int(o["ate"][0][19]) == 0
        assert np.abs(o["ate"][0][7:16].reshape(3, 3) - Rw.T).max() < 1e-13
    assert tn.evaluate(moved, 30, G, align="none", gt_kind="c2w")["ate"][0][2] > 1.0


# ------------------------------------------------------------------------------------------------ 3. prefixes and the segment search
@pytest.mark.parametrize("cap", [1, 255, 256, 257, 1000, 4096])
def test_prefix_against_fsum_and_search_against_a_scan(cap):
    rng = np.random.default_rng(cap)
    steps = rng.random(cap) * 2.0
    steps[rng.random(cap) < 0.2] = 0.0                              # unused rows and standstills add nothing
    dist = tn.blocked_prefix(steps, cap)
    Cb = -(-cap // 256)
    assert (np.diff(dist) >= 0).all()
    for i in sorted(set(rng.integers(0, cap, 40).tolist() + [0, cap - 1])):
        exact = math.fsum(steps[:i + 1])
        assert abs(dist[i] - exact) <= (Cb + 257) * EPS * exact, (i, dist[i], exact)
    n = max(cap - 3, 1)
    for f in sorted(set(rng.integers(0, n, 30).tolist())):
        later = dist[f + 1:n][dist[f + 1:n] > dist[f]]
        lens = [0.3, 5.0, 1e9] + ([float(later[0] - dist[f])] if len(later) else [])      # the last: a prefix value met exactly
        for length in lens:
            j = tn.segment_end(dist, n, f, length)
            assert j == tn.segment_end_scan(dist, n, f, length) and j > f, (f, length)
            if len(lens) == 4 and length == lens[3] and dist[f] + length == later[0]:
                k = f + 1 + int(np.argmax(dist[f + 1:n] > dist[f]))           # the first row that meets the length exactly ..
                assert dist[k] == later[0] and j > k                          # .. does not end the segment: the comparison is strict


def test_tree_sum_is_the_stated_tree():
    rng = np.random.default_rng(5)
    for M in (0, 1, 255, 256, 257, 1000):
        x = rng.normal(size=M) * 1e3
        lanes = [0.0] * 256
        for i in range(M):
            lanes[i % 256] = lanes[i % 256] + float(x[i])
        s = 128
        while s:
            for t in range(s):
                lanes[t] = lanes[t] + lanes[t + s]
            s //= 2
        assert tn.tree_sum(x) == lanes[0]
        assert abs(tn.tree_sum(x) - math.fsum(x)) <= (M / 256 + 9) * EPS * float(np.abs(x).sum()) + 0.0


# ------------------------------------------------------------------------------------------------ 4. metrics on synthetic drives
def test_rpe_and_segments_of_a_scaled_copy():
    G = tn.drive(400, 11, spacing=1.0, standstill=range(100, 110))
    est = tn.perturb(G, 0, noise=0.0, scale=0.9)                    # a world shrunk by 0.9: rotations right, translations 10 % short
    o = tn.evaluate(est, 400, G, align="none", gt_kind="c2w", deltas=(1, 7, 399, 400, 405), lengths=(0.5, 50.0, 1e6), step=10)
    r = o["rpe"][0]
    assert r[:, 0].tolist() == [399, 393, 1, 0, 0] and not r[3:].any()
    assert abs(r[0, 2] - 0.1 * 389 / 399) < 1e-9 and r[0, 6] < 1e-7  # 389 moving steps of 1 m, each 0.1 m short; no rotation error
    s = o["seg"][0]
    assert s[2, 0] == 0 and (o["seg_end"][0][:, 2] == -1).all()     # longer than the whole path
    assert s[0, 0] == 40 and abs(s[0, 3] - 0.9) < 1e-12 and abs(s[1, 3] - 0.9) < 1e-12
    ends = o["seg_end"][0][:, 0]
    assert ends[10] == 110 and ends[9] == 91                        # the start inside the standstill ends behind it: no zero-length segment
    assert s[3, 0] == s[0, 0] + s[1, 0] and 0.08 < s[1, 1] < 0.1   # 10 % of the chord, which is a little shorter than the path
    sim = tn.evaluate(est, 400, G, align="sim3", gt_kind="c2w", deltas=(1,), lengths=(50.0,), step=10)
    assert abs(sim["ate"][0][6] - 1 / 0.9) < 1e-12 and sim["ate"][0][2] < 1e-11 and sim["rpe"][0][0, 2] < 1e-11 and sim["seg"][0][0, 1] < 1e-12


def test_closure_rule():
    G = tn.drive(50, 4)
    W = tn.invert_rows(G)
    R, t = tn.split(W)
    pairs = [(3, 40), (10, 45), (5, 5), (-1, 7), (7, 50), (8, 20), (2, 30), (12, 33)]
    Z = np.zeros((10, 12))
    for a, (i, j) in enumerate(pairs):
        if 0 <= i < 50 and 0 <= j < 50:
            Rz, tz = tn.rigid_mul(R[i], t[i], *tn.rigid_inv(R[j], t[j]))
            Z[a] = np.hstack([Rz, tz[:, None]]).reshape(-1)
    Z[1, 3] += 0.5                                                  # 0.5 m off
    Z[5, 7] = np.nan
    gt = G.copy()
    gt[30, 2] = np.inf                                              # edge 6 loses its gt row
    eij = np.zeros((10, 2), np.int32)
    eij[:8] = pairs
    o = tn.evaluate(W, 50, gt, align="none", gt_kind="c2w", log=(eij, Z, np.array([8, 0, 0, 0])), edge_capacity=10, rot_thr=0.01, trans_thr=0.25)
    ee = o["edge_err"]
    assert (ee[[2, 3, 4, 5, 6, 8, 9]] == -1).all() and (ee[[0, 1, 7]] >= 0).all()
    assert o["clo"][0] == 3 and o["clo"][1] == 1 and o["clo"][6] == 8 and abs(ee[1, 1] - 0.5) < 1e-12 and ee[0, 1] < 1e-12 and ee[7, 0] < 1e-7
    assert abs(o["clo"][5] - 0.5) < 1e-12 and abs(o["clo"][4] - 0.5 / math.sqrt(3)) < 1e-12


# ------------------------------------------------------------------------------------------------ 5. the committed sequences
def load_seq(name):
    d = os.path.join(SEQ, name)
    ids, poses = ev.load_pose_history(d)
    inc = np.loadtxt(os.path.join(d, "incoming_id_file.txt")).astype(np.int64)
    sel = np.isin(ids, inc)
    assert np.array_equal(ids[sel], inc)                            # the poses that became clouds, in file order
    return poses[sel], ev.load_kitti_gt_poses(d)


@pytest.mark.parametrize("name,rows", [("kitti_seq07", 693), ("kitti_seq06", 880)])
def test_the_committed_sequences_through_the_restatement(name, rows):
    est, gt = load_seq(name)
    assert est.shape == (rows, 12) and gt.shape == (rows, 12)
    assert np.array_equal(gt[:, [3, 7, 11]], ev.load_kitti_ground_truth(os.path.join(SEQ, name)))
    res = {}
    for mode in ("none", "first", "se3", "sim3"):
        o = tn.evaluate(est, rows, gt, align=mode, gt_kind="c2w", deltas=(1, 10), lengths=tuple(100.0 * k for k in range(1, 9)))
        a = o["ate"][0]
        res[mode] = a[2]
        print(f"   {name} {mode}: N {a[0]:.0f} ATE rmse {a[2]:.4f} mean {a[3]:.4f} max {a[4]:.4f} at {a[5]:.0f} s {a[6]:.5f} flags {a[19]:.0f}")
        if mode in ("se3", "sim3"):
            for k, dl in enumerate((1, 10)):
                r = o["rpe"][0][k]
                print(f"      RPE delta {dl}: pairs {r[0]:.0f} trans rmse {r[1]:.4f} mean {r[2]:.4f} max {r[3]:.4f} rot rmse {r[4]:.5f} mean {r[5]:.5f}")
            for l in range(9):
                s = o["seg"][0][l]
                print(f"      seg {'all' if l == 8 else 100 * (l + 1)}: n {s[0]:.0f} t_err {100 * s[1]:.3f} % r_err {s[2]:.3e} rad/m ratio {s[3]:.4f}")
        assert a[0] == rows and int(a[19]) == 0 and np.isfinite(o["ate"]).all() and np.isfinite(o["rpe"]).all() and np.isfinite(o["seg"]).all()
    assert res["sim3"] <= res["se3"] <= res["first"] + 1e-9 and res["se3"] <= res["none"]      # each alignment has the freedom of the one before
