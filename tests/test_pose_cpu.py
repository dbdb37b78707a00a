"""CPU checks of the pose seeds (pr_relative_pose, csrc/pose_seed.hpp) against the restatement pose_np.py and the reference's own files:
the header and bindings, argument errors without a device, SC bit-equality with pr_sc_relative_pose, the M2DP / DELIGHT sign tables
against test_m2dp.cpp's loop order and processDELIGHT.m's Mut, recovery of a known rigid motion from the oracle's signatures, and the
rule that chooses among refined hypotheses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib
import pose_np
from resident_fuzz_cases import bits_equal
from so_dso_place_recognition_amd import _lib, api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = (("sc", pose_np.SC), ("m2dp", pose_np.M2DP), ("delight", pose_np.DELIGHT))


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def random_frames(rng, c, left=None):
    """c frames with random orthonormal E (left-handed where left[i], random handedness by default), mean ~ 3 m, 100 points."""
    f = np.zeros((c, 16))
    for i in range(c):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        want_left = rng.random() < 0.5 if left is None else left[i]
        if (np.linalg.det(Q) < 0) != want_left:
            Q[:, 0] = -Q[:, 0]
        f[i, :3] = rng.normal(0, 3, 3)
        f[i, 3:12] = Q.T.reshape(-1)
        f[i, 13] = 100
    return f


def ident_frame(c=1):
    f = np.zeros((c, 16)); f[:, 3:12] = np.eye(3).reshape(-1); f[:, 13] = 10
    return f


# ------------------------------------------------------------------------------------------ a. header, bindings, argument errors
def test_header_and_bindings_declare_the_pose_entry_points():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for name, val in (("PR_POSE_SC", 0), ("PR_POSE_M2DP", 1), ("PR_POSE_DELIGHT", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), txt), name
    lib = _lib.load()
    for fn in ("pr_relative_pose", "pr_relative_pose_dev", "pr_verify_pairs_dev", "pr_verify_select_dev"):
        assert fn in _lib.SYMBOLS and hasattr(lib, fn) and re.search(r"\bint %s\(" % fn, txt), fn
    assert (_lib.POSE_SC, _lib.POSE_M2DP, _lib.POSE_DELIGHT) == (0, 1, 2)
    for f in ("relative_pose", "relative_pose_torch", "verify_pairs_torch"):
        assert callable(getattr(api, f))
    from so_dso_place_recognition_amd import matcher
    assert callable(matcher._Base.verify_dev)


def test_host_form_rejects_bad_inputs():
    lib = _lib.load()
    f = ident_frame(); T = np.empty((1, 3, 4))
    ok = np.array([1], np.int32)
    for bad_type in (-1, 3):
        assert lib.pr_relative_pose(bad_type, p(f), p(f), p(ok), 1, p(T)) == _lib.PR_EINVAL
        assert b"type" in lib.pr_last_error(None)
    for name, t in TYPES:
        for bad in (-1, pose_np.VARIANTS[t], 1000):
            v = np.array([bad], np.int32)
            assert lib.pr_relative_pose(t, p(f), p(f), p(v), 1, p(T)) == _lib.PR_EINVAL
            assert b"variant" in lib.pr_last_error(None)
        few = f.copy(); few[0, 13] = 2
        assert lib.pr_relative_pose(t, p(f), p(few), p(ok), 1, p(T)) == _lib.PR_EINVAL
        assert lib.pr_relative_pose(t, p(few), p(f), p(ok), 1, p(T)) == _lib.PR_EINVAL
        assert lib.pr_relative_pose(t, p(f), p(f), p(ok), 1, p(T)) == _lib.PR_OK
        assert lib.pr_relative_pose(t, None, None, None, 0, None) == _lib.PR_OK
        assert lib.pr_relative_pose(t, None, p(f), p(ok), 1, p(T)) == _lib.PR_EINVAL
        with pytest.raises(_lib.PRError):
            api.relative_pose(name, f, f, [pose_np.VARIANTS[t]])
    with pytest.raises(ValueError):
        api.relative_pose("gist", f, f, [0])


def test_device_forms_reject_bad_arguments_before_any_device_is_touched():
    """No context and no device: every argument error is PR_EINVAL with its text; the buffers are never read."""
    lib = _lib.load()
    buf = np.zeros(64)
    b = p(buf)

    def seed(type_=0, m=2, n=3, k=1, stride=2, H=1, fq=b, idx=b):
        return lib.pr_relative_pose_dev(None, type_, fq, m, b, n, 0, k, idx, b, stride, H, b, b, b)

    def verify(type_=0, m=2, k=1, stride=2, H=1, max_iter=30, max_corr=1.0, min_inl=3, min_fit=0.5, max_src=100, offs=b):
        return lib.pr_verify_pairs_dev(None, type_, b, offs, 2, b, b, 3, b, b, m, 3, 0, k, b, b, stride, H, max_src, 100, max_iter, max_corr, 1e-6,
                                       1e-6, min_inl, min_fit, 0.5, b, b, b, b)
    for call, text in ((lambda: seed(type_=3), b"type"), (lambda: seed(m=-1), b"negative"), (lambda: seed(H=0), b"H="), (lambda: seed(H=3), b"H="),
                       (lambda: seed(type_=2, H=2), b"DELIGHT"), (lambda: seed(stride=1, H=2), b"variant_stride"),
                       (lambda: seed(m=300, k=200, H=2, stride=2), b"65535"), (lambda: seed(fq=None), b"NULL"), (lambda: seed(idx=None), b"NULL"),
                       (lambda: seed(), b"ctx is NULL"),
                       (lambda: verify(type_=-1), b"type"), (lambda: verify(H=3), b"H="), (lambda: verify(stride=0), b"variant_stride"),
                       (lambda: verify(m=40000, k=1, H=2), b"65535"), (lambda: verify(max_iter=-1), b"max_iter"),
                       (lambda: verify(max_corr=0.0), b"max_corr"), (lambda: verify(min_inl=2), b"min_inliers"),
                       (lambda: verify(min_fit=float("nan")), b"NaN"), (lambda: verify(max_src=-1), b"negative"), (lambda: verify(offs=None), b"NULL"),
                       (lambda: verify(), b"ctx is NULL")):
        assert call() == _lib.PR_EINVAL
        assert text in lib.pr_last_error(None), (text, lib.pr_last_error(None))
    assert lib.pr_verify_select_dev(None, b, b, 4, 0, 0.5, 0.5, b, b, b, b) == _lib.PR_EINVAL
    assert lib.pr_verify_select_dev(None, b, b, 4, 2, 0.5, 0.5, b, b, b, b) == _lib.PR_EINVAL and b"ctx is NULL" in lib.pr_last_error(None)


# ------------------------------------------------------------------------------------------ b. SC: the bits of pr_sc_relative_pose
def test_sc_seed_equals_pr_sc_relative_pose_bit_for_bit():
    rng = np.random.default_rng(31)
    fq, fd = random_frames(rng, 8), random_frames(rng, 8)
    worst = 0.0
    for v in range(120):
        var = np.full(8, v, np.int32)
        a = api.relative_pose("sc", fq, fd, var)
        b = api.sc_relative_pose(fq, fd, var)
        assert bits_equal(a, b), v
        for i in range(8):
            w = pose_np.relative_pose(pose_np.SC, fq[i], fd[i], v)
            worst = max(worst, float(np.abs(a[i] - w).max()))
            assert abs(np.linalg.det(a[i][:, :3]) - 1) < 1e-12
    print("   SC: library against pose_np, max |dT| %.2e" % worst)
    assert worst <= 1e-14


@pytest.mark.parametrize("name,t", TYPES[1:])
def test_m2dp_and_delight_seeds_equal_the_restatement_and_are_proper(name, t):
    rng = np.random.default_rng(32)
    fq, fd = random_frames(rng, 8), random_frames(rng, 8)
    for v in range(pose_np.VARIANTS[t]):
        a = api.relative_pose(name, fq, fd, np.full(8, v, np.int32))
        for i in range(8):
            assert np.abs(a[i] - pose_np.relative_pose(t, fq[i], fd[i], v)).max() <= 1e-14
            R = a[i][:, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
            assert np.abs(R @ fq[i, :3] + a[i][:, 3] - fd[i, :3]).max() < 1e-12          # the centroid maps onto the centroid


# ------------------------------------------------------------------------------------------ c. the sign tables
def test_m2dp_table_is_the_generators_loop_order():
    rows = []
    for direction_x in range(-1, 2, 2):                      # test_m2dp.cpp:47-48
        for direction_y in range(-1, 2, 2):
            rows.append(np.diag([direction_x, direction_y, direction_x * direction_y]).astype(np.float64))   # :54-55
    f = ident_frame()
    seen = set()
    for a in range(4):
        for b in range(4):
            assert np.array_equal(pose_np.m2dp_D(a), rows[a])
            S0 = rows[b] @ rows[a]
            T = api.relative_pose("m2dp", f, f, [4 * a + b])[0]
            assert np.array_equal(T[:, :3], S0) and np.array_equal(T[:, 3], np.zeros(3)), (a, b)
            assert np.linalg.det(S0) == 1.0
            # the match says D_a q' ~ D_b d': the seed's d' = S0 q' satisfies it
            q = np.array([0.3, -1.2, 2.5])
            assert np.array_equal(rows[a] @ q, rows[b] @ (S0 @ q))
            seen.add(tuple(np.diag(S0)))
    assert len(seen) == 4


def test_delight_table_is_mut():
    Mut = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16],          # processDELIGHT.m:2-5
                    [6, 5, 8, 7, 2, 1, 4, 3, 14, 13, 16, 15, 10, 9, 12, 11],
                    [7, 8, 5, 6, 3, 4, 1, 2, 15, 16, 13, 14, 11, 12, 9, 10],
                    [4, 3, 2, 1, 8, 7, 6, 5, 12, 11, 10, 9, 16, 15, 14, 13]]) - 1

    def octant(v):                                                                    # DELIGHT.cpp:21
        return 4 * (v[2] > 0) + 2 * (v[1] > 0) + 1 * (v[0] > 0)
    f = ident_frame()
    want = ([1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1])
    for k in range(4):
        S0 = api.relative_pose("delight", f, f, [k])[0][:, :3]
        assert np.array_equal(S0, np.diag(want[k]).astype(np.float64)) and np.array_equal(S0, pose_np.delight_S0(k))
        for o in range(8):
            q = np.array([1.0 if o & 1 else -1.0, 1.0 if o & 2 else -1.0, 1.0 if o & 4 else -1.0])
            assert octant(q) == o
            # row o of Bk is row Mut[k, o] of B: the query's octant o meets the entry's octant Mut[k, o], which is where S0 sends it
            assert octant(S0 @ q) == Mut[k, o] == (o ^ pose_np.DELIGHT_XOR[k])
            assert Mut[k, o + 8] == 8 + Mut[k, o]


# ------------------------------------------------------------------------------------------ d. recovery of a known motion
SIGNS = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _m2dp_rows(al, inten):
    """The oracle's signature rows of aligned points (test_m2dp.cpp:46-66 with M2DP.cpp's matrices and leading singular pairs)."""
    rows = []
    for dx, dy in pose_np.M2DP_DIRS:
        cm, im = oracle_lib.m2dp_matrices(al, inten, 45.0, int(dx), int(dy))
        rows.append(np.concatenate([oracle_lib.top_singular_pair(cm), oracle_lib.top_singular_pair(im)]))
    return np.array(rows)


def _delight_rows(al, inten):
    """DELIGHT.cpp:14-23 on aligned points (the reference's float arithmetic)."""
    a = al.astype(np.float32)
    d = np.linalg.norm(al, axis=1).astype(np.float32)
    hist = 8 * (d > np.float32(10.0)) + 4 * (a[:, 2] > 0) + 2 * (a[:, 1] > 0) + 1 * (a[:, 0] > 0)
    out = np.zeros((16, 256))
    np.add.at(out, (hist, inten.astype(np.int64)), 1.0)
    return out


def _recovery_cases():
    """6 scene clouds and their rigid copies; the copy's frame is the query's moved by the motion, with each of the 8 sign patterns."""
    for i in range(6):
        xyz, inten = synth.scene_cloud(77, i, 2000)
        R = _rot((0, -1, 0), 17.0 + 60.0 * i) @ _rot((np.cos(i), 0, np.sin(i)), 5.0 * (i + 1) / 6)
        t = np.array([3.0 - i, 0.2 * i - 0.5, -2.0 + 1.5 * i])
        d = xyz @ R.T + t
        fq = pose_np.frame(xyz)
        base = pose_np.frame(d)
        flip = np.sign(np.sum(pose_np.E_of(base) * (R @ pose_np.E_of(fq)), 0))      # the solver's signs, undone: E_d = R E_q
        for s in SIGNS:
            yield i, xyz, inten, d, R, t, fq, pose_np.frame(d, signs=flip * np.array(s)), s


def test_seeds_recover_a_known_motion_from_the_oracles_signatures():
    near = {"m2dp": 0, "delight": 0}
    improper = 0
    worst = {"m2dp": [0.0, 0.0], "delight": [0.0, 0.0]}
    cache = {}
    for i, xyz, inten, d, R, t, fq, fd, s in _recovery_cases():
        if i not in cache:
            al = pose_np.aligned(xyz, fq)
            cache[i] = (_m2dp_rows(al, inten), _delight_rows(al, inten))
        q_m2, q_dl = cache[i]
        ald = pose_np.aligned(d, fd)
        v_m2, blk = pose_np.m2dp_variant(q_m2, _m2dp_rows(ald, inten))
        v_dl, dist = pose_np.delight_variant(q_dl, _delight_rows(ald, inten))
        proper = s[0] * s[1] * s[2] > 0
        improper += not proper
        for name, v, d0 in (("m2dp", v_m2, blk.reshape(-1)[v_m2]), ("delight", v_dl, dist[v_dl])):
            T = api.relative_pose(name, fq[None], fd[None], [v])[0]
            Rg, tg = T[:, :3], T[:, 3]
            if proper:
                eR, et = np.abs(Rg - R).max(), np.abs(tg - t).max() / (1 + np.linalg.norm(fq[:3]))
                worst[name] = [max(worst[name][0], eR), max(worst[name][1], et)]
                assert eR <= 1e-9 and et <= 1e-9, (name, i, s, v, eR, et)
                # an exact copy: the right variant's distance is the formula's minimum - 0 for DELIGHT's chi-square; (1 - 2) / 2 for
                # processM2DP.m:15, whose rows are two unit vectors U1 | V1 side by side
                assert abs(d0 - (-0.5 if name == "m2dp" else 0.0)) <= 1e-9, (name, i, s, d0)
            else:
                assert np.abs(Rg @ Rg.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rg) - 1) <= 1e-12
                ang = np.degrees(np.arccos(np.clip((np.trace(Rg.T @ R) - 1) / 2, -1, 1)))
                near[name] += ang <= 5.0
    print("   proper patterns: worst |dR|, |dt| / (1 + |mu|):", worst)
    print("   improper patterns: seeds within 5 degrees: m2dp %d / %d, delight %d / %d" % (near["m2dp"], improper, near["delight"], improper))


# ------------------------------------------------------------------------------------------ e. the select rule
def stats_rec(rows):
    """rows of (fitness, rmse, status) -> records of api.ICP_STATS."""
    s = np.zeros(len(rows), api.ICP_STATS)
    for i, (f, r, st) in enumerate(rows):
        s[i] = (f, r, 100, 5, st, 0)
    return s


NAN = float("nan")
# (hypotheses' (fitness, rmse, status), min_fitness, max_rmse) -> (hyp, accepted)
SELECT_CASES = [
    ([(0.9, 0.1, 0), (0.8, 0.05, 0)], 0.5, 0.5, (0, True)),                 # the larger fitness
    ([(0.8, 0.1, 0), (0.9, 0.2, 1)], 0.5, 0.5, (1, True)),                  # ... whichever slot holds it; max_iter qualifies
    ([(0.8, 0.2, 0), (0.8, 0.1, 0)], 0.5, 0.5, (1, True)),                  # equal fitness: the smaller rmse
    ([(0.8, 0.1, 0), (0.8, 0.1, 0)], 0.5, 0.5, (0, True)),                  # a full tie: the smaller h
    ([(0.9, 0.1, 2), (0.6, 0.3, 0)], 0.5, 0.5, (1, True)),                  # too_few does not qualify
    ([(0.9, 0.1, 3), (0.9, 0.1, 4)], 0.5, 0.5, (0, False)),                 # none qualifies: hypothesis 0, not accepted
    ([(0.0, 0.0, 4), (0.0, 0.0, 4)], 0.0, 0.5, (0, False)),                 # ... even where the thresholds would pass
    ([(NAN, 0.1, 0), (0.2, 0.3, 0)], 0.1, 0.5, (1, True)),                  # a NaN fitness loses to a number
    ([(0.2, 0.3, 0), (NAN, 0.1, 0)], 0.1, 0.5, (0, True)),
    ([(NAN, 0.1, 0), (NAN, 0.05, 0)], 0.1, 0.5, (0, False)),                # only NaNs: the first, not accepted
    ([(0.8, NAN, 0), (0.8, 0.4, 0)], 0.5, 0.5, (1, True)),                  # equal fitness: a NaN rmse loses to a number
    ([(0.8, 0.4, 0), (0.8, NAN, 0)], 0.5, 0.5, (0, True)),
    ([(0.8, NAN, 0), (0.7, 0.1, 4)], 0.5, 0.5, (0, False)),                 # the only qualified one has a NaN rmse: kept, not accepted
    ([(0.4, 0.1, 0), (0.3, 0.1, 0)], 0.5, 0.5, (0, False)),                 # below min_fitness
    ([(0.9, 0.6, 0), (0.8, 0.7, 1)], 0.5, 0.5, (0, False)),                 # above max_rmse
    ([(0.5, 0.5, 0), (0.1, 0.1, 0)], 0.5, 0.5, (0, True)),                  # the thresholds are inclusive
    ([(0.7, 0.2, 1)], 0.5, 0.5, (0, True)),                                 # H = 1
    ([(0.7, 0.2, 2)], 0.5, 0.5, (0, False)),
]


def test_select_rule_on_hand_made_statistics():
    for rows, mf, mr, want in SELECT_CASES:
        assert pose_np.select(stats_rec(rows), mf, mr) == want, rows
