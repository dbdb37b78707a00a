"""The loop-closure log and the pose-graph relaxation (pr_posegraph) without a device: the ABI surface, the argument errors
that are returned before any device is touched, and the properties of the NumPy restatement the GPU tests compare the kernels with
(posegraph_np.py) - its analytic Jacobians against central differences, the add rule slot by slot, what the skipped edges and the gauge
do, and that the consistent graph recovers ground truth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import posegraph_np as pg
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pr_posegraph_create", "pr_posegraph_destroy", "pr_posegraph_reset", "pr_posegraph_count", "pr_posegraph_add_dev", "pr_posegraph_add",
         "pr_posegraph_relax_dev")
OVERFLOW = pg.OVERFLOW


def test_posegraph_symbols_records_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_posegraph_")) == sorted(NAMES)
    assert re.search(r"#define\s+PR_POSEGRAPH_OVERFLOW\s+1\b", code) and _lib.POSEGRAPH_OVERFLOW == 1 == OVERFLOW
    assert _lib.POSEGRAPH_MAX_K == pg.MAX_K == 128
    assert "typedef struct pr_posegraph pr_posegraph;" in code
    fields = re.search(r"typedef struct pr_posegraph_buffers \{(.*?)\} pr_posegraph_buffers;", code, flags=re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)\s*;", fields)) == tuple(n for n, _ in _lib.PoseGraphBuffers._fields_) == api.PoseGraph.NAMES
    assert C.sizeof(_lib.PoseGraphBuffers) == 4 * C.sizeof(C.c_void_p)
    prm = re.search(r"typedef struct pr_posegraph_params \{(.*?)\} pr_posegraph_params;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", prm.strip()) == "int32_t outer, inner; double lambda, w_odo_rot, w_odo_trans;"
    assert [n for n, _ in _lib.PoseGraphParams._fields_] == ["outer", "inner", "lambda", "w_odo_rot", "w_odo_trans"]
    assert [t for _, t in _lib.PoseGraphParams._fields_] == [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]
    assert C.sizeof(_lib.PoseGraphParams) == 32 and _lib.PoseGraphParams.w_odo_trans.offset == 24
    for m in ("add_torch", "add", "relax_torch", "relax_map", "reset", "count", "close"):
        assert hasattr(api.PoseGraph, m), m
    assert "pr_posegraph" in txt and "DESIGN.md 4.17" in txt and "tests/posegraph_np.py" in txt


def _bufs(null=None):
    """a pr_posegraph_buffers of non-NULL addresses that are never dereferenced (every case below fails before the device is touched)"""
    store = (C.c_double * 8)()
    b = _lib.PoseGraphBuffers(*([C.addressof(store)] * 4))
    if null:
        setattr(b, null, None)
    return b, store


@pytest.mark.parametrize("args,word", [
    ((0, 8, 4, 16), "node_capacity=0"), ((-2, 8, 4, 16), "node_capacity=-2"), (((1 << 20) + 1, 8, 4, 16), "node_capacity="),
    ((8, 0, 4, 16), "edge_capacity=0"), ((8, (1 << 20) + 1, 4, 16), "edge_capacity="),
    ((8, 8, 0, 16), "max_outer=0"), ((8, 8, 65, 16), "max_outer=65"),
    ((8, 8, 4, 0), "max_inner=0"), ((8, 8, 4, (1 << 16) + 1), "max_inner="),
    ((8, 8, 4, 16), "ctx is NULL"), ((1 << 20, 1 << 20, 64, 1 << 16), "ctx is NULL")])
def test_posegraph_create_argument_errors(args, word):
    """Value checks come before anything touches a device.  (The NULL context is the last check: a valid argument set reaches it.)"""
    lib = _lib.load()
    b, keep = _bufs()
    h = C.c_void_p(1)
    assert lib.pr_posegraph_create(None, C.byref(b), *args, C.byref(h)) == _lib.PR_EINVAL and not h.value
    msg = lib.pr_last_error(None).decode()
    assert "pr_posegraph_create" in msg and word in msg, msg


@pytest.mark.parametrize("name", api.PoseGraph.NAMES)
def test_posegraph_create_null_buffer(name):
    lib = _lib.load()
    b, keep = _bufs(null=name)
    h = C.c_void_p(1)
    assert lib.pr_posegraph_create(None, C.byref(b), 8, 8, 4, 16, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert b"a buffer is NULL" in lib.pr_last_error(None)


def test_posegraph_null_handles_and_values():
    lib = _lib.load()
    b, keep = _bufs()
    n, f = C.c_int32(7), C.c_int32(7)
    buf = (C.c_double * 64)()
    err = lambda: lib.pr_last_error(None)
    assert lib.pr_posegraph_create(None, C.byref(b), 8, 8, 4, 16, None) == _lib.PR_EINVAL and b"out is NULL" in err()
    h = C.c_void_p(1)
    assert lib.pr_posegraph_create(None, None, 8, 8, 4, 16, C.byref(h)) == _lib.PR_EINVAL and b"buffers is NULL" in err()
    assert lib.pr_posegraph_reset(None) == _lib.PR_EINVAL and b"pr_posegraph_reset" in err()
    assert lib.pr_posegraph_count(None, C.byref(n), C.byref(f)) == _lib.PR_EINVAL and b"pr_posegraph_count" in err()
    add_dev = lambda k, wr, wt: lib.pr_posegraph_add_dev(None, buf, buf, buf, buf, k, wr, wt, buf)
    assert add_dev(1, 1.0, 1.0) == _lib.PR_EINVAL and b"pr_posegraph_add_dev: graph is NULL" in err()
    for k in (0, -1, 129):
        assert add_dev(k, 1.0, 1.0) == _lib.PR_EINVAL and b"k=%d outside" % k in err()
    for w in (float("nan"), float("inf"), -1.0):
        assert add_dev(1, w, 1.0) == _lib.PR_EINVAL and b"w_rot is negative or not finite" in err()
        assert add_dev(1, 1.0, w) == _lib.PR_EINVAL and b"w_trans is negative or not finite" in err()
    add = lambda k: lib.pr_posegraph_add(None, buf, buf, buf, 0, k, 1.0, 1.0, buf)
    assert add(1) == _lib.PR_EINVAL and b"pr_posegraph_add: graph is NULL" in err()
    assert add(0) == _lib.PR_EINVAL and b"k=0 outside" in err() and add(129) == _lib.PR_EINVAL and b"k=129 outside" in err()
    relax = lambda *p: lib.pr_posegraph_relax_dev(None, buf, buf, C.byref(_lib.PoseGraphParams(*p)), buf, buf)
    assert relax(1, 1, 0.0, 1.0, 1.0) == _lib.PR_EINVAL and b"pr_posegraph_relax_dev: graph is NULL" in err()
    assert lib.pr_posegraph_relax_dev(None, buf, buf, None, buf, buf) == _lib.PR_EINVAL and b"params is NULL" in err()
    for o in (0, -3):
        assert relax(o, 1, 0.0, 1.0, 1.0) == _lib.PR_EINVAL and b"outer=%d" % o in err()
        assert relax(1, o, 0.0, 1.0, 1.0) == _lib.PR_EINVAL and b"inner=%d" % o in err()
    for w in (float("nan"), float("inf"), -float("inf"), -1e-300):
        assert relax(1, 1, w, 1.0, 1.0) == _lib.PR_EINVAL and b"lambda is negative or not finite" in err()
        assert relax(1, 1, 0.0, w, 1.0) == _lib.PR_EINVAL and b"w_odo_rot is negative or not finite" in err()
        assert relax(1, 1, 0.0, 1.0, w) == _lib.PR_EINVAL and b"w_odo_trans is negative or not finite" in err()
    lib.pr_posegraph_destroy(None)                     # a no-op


def test_pose_graph_refuses_another_context_before_the_library():
    class Fake:
        pass
    g = api.PoseGraph.__new__(api.PoseGraph)           # no handle, no library call: the check is the first thing relax_map does
    g.ctx, g.node_capacity, g.h = object(), 8, None
    km = Fake(); km.ctx, km.keyframe_capacity = object(), 8
    with pytest.raises(ValueError, match="share one context"):
        g.relax_map(km)
    km.ctx, km.keyframe_capacity = g.ctx, 9
    with pytest.raises(ValueError, match="node_capacity"):
        g.relax_map(km)


# ------------------------------------------------------------------------------------------------ the restatement's Jacobians
def _rand_pose(rng):
    P = np.zeros((3, 4))
    P[:, :3] = pg.exp_so3(rng.normal(0.0, 1.0, 3))
    P[:, 3] = rng.normal(0.0, 5.0, 3)
    return P


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-3, 1.0, 2.0])
@pytest.mark.parametrize("side", [0, 1])
def test_jacobians_against_central_differences(angle, side):
    """A = dr / d delta_i and B = dr / d delta_j at delta = 0 against central differences with h = 1e-6: agreement to 1e-7 relative (the
    truncation term h^2 f''' and the rounding term eps / h are both about 1e-10).  The edge's residual rotation has the given angle."""
    rng = np.random.default_rng(int(angle * 1000) + 7)
    Pi, Pj = _rand_pose(rng), _rand_pose(rng)
    ax = rng.normal(0.0, 1.0, 3)
    ax /= np.linalg.norm(ax)
    E = np.zeros((3, 4))
    E[:, :3] = pg.exp_so3(ax * angle)
    E[:, 3] = rng.normal(0.0, 1.0, 3)
    Z = pg.mul(pg.mul(Pi, pg.inv(Pj)), pg.inv(E))      # Z^-1 P_i P_j^-1 = E
    r, A, B = pg.linearize(Z[None], Pi[None], Pj[None])
    assert abs(np.linalg.norm(r[0, :3]) - angle) < 1e-12
    Jm, h = (A[0], B[0])[side], 1e-6
    fd = np.zeros((6, 6))
    for c in range(6):
        d = np.zeros((1, 6))
        d[0, c] = h
        hi, lo = [Pi[None], Pj[None]], [Pi[None], Pj[None]]
        hi[side], lo[side] = pg.update(hi[side], d), pg.update(lo[side], -d)
        fd[:, c] = (pg.linearize(Z[None], hi[0], hi[1], jac=False)[0] - pg.linearize(Z[None], lo[0], lo[1], jac=False)[0]) / (2 * h)
    rel = np.abs(fd - Jm).max() / np.abs(Jm).max()
    print("   angle", angle, "side", side, "rel", rel)
    assert rel < 1e-7


# ------------------------------------------------------------------------------------------------ the add rule
def test_add_rule_slot_by_slot():
    m = pg.PoseGraphModel(4)
    T = np.arange(5 * 12, dtype=np.float64).reshape(5, 12)
    T[3, 7] = np.nan
    #            not accepted, no row, the query's own row, NaN in T, logged
    info = m.add([3, -1, 9, 2, 5], T, [0, 1, 1, 1, 1], 9, 2.0, 3.0)
    assert info.tolist() == [1, 0, 1, 0] and m.state.tolist() == [1, 0, 0, 0]
    assert m.edge_ij[0].tolist() == [5, 9] and np.array_equal(m.edge_Z[0], T[4]) and m.edge_w[0].tolist() == [2.0, 3.0]
    before = [a.copy() for a in (m.edge_ij, m.edge_Z, m.edge_w, m.state)]
    assert m.add([1, 2], T[:2], [1, 1], -1).tolist() == [0, -1, 1, 0]          # a negative query row switches the call off
    assert all(np.array_equal(a, b) for a, b in zip(before, (m.edge_ij, m.edge_Z, m.edge_w, m.state)))
    assert m.add([0, 1], T[:2], [1, 1], 10).tolist() == [2, 1, 3, 0]            # slots in ascending order
    assert m.edge_ij[1:3].tolist() == [[0, 10], [1, 10]]
    assert m.add([4, 6, 7], T[:3], [1, 1, 1], 11).tolist() == [1, 3, 4, OVERFLOW]   # one fits, two do not
    assert m.edge_ij[3].tolist() == [4, 11]
    assert m.add([1], T[:1], [0], 12).tolist() == [0, -1, 4, OVERFLOW]          # the flag stays in every later info
    assert m.add([1], T[:1], [1], -5).tolist() == [0, -1, 4, OVERFLOW]
    m.state[0] = 99                                                             # a scribbled count is clamped
    assert m.add([1], T[:1], [1], 12).tolist() == [0, -1, 4, OVERFLOW]
    m.reset()
    assert m.state.tolist() == [0, 0, 0, 0] and m.add([1], T[:1], [1], 12).tolist() == [1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ properties of the relaxation
def _same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_an_empty_log_returns_the_poses_bit_for_bit():
    c = pg.noisy_case(12, 3, 1)
    poses = c["poses"].copy()
    poses[4, 2] = -0.0                                 # a negative zero survives
    m = pg.PoseGraphModel(4)
    for n in (0, 1, 2, 12):
        out, rep = pg.relax(poses, n, m.edge_ij, m.edge_Z, m.edge_w, 0, 3, 8, 1e-9, 100.0, 10.0)
        assert _same_bytes(out, poses) and not rep[:4].any() and rep[4] == max(n - 1, 0), n
    assert _same_bytes(pg.update(poses, np.zeros((12, 6))).reshape(12, 12), poses)              # a zero delta is the identity


def test_node_zero_never_moves_and_rows_behind_n_are_kept():
    c = pg.noisy_case(12, 3, 1)
    m = pg.log_of(c)
    out, rep = pg.relax(c["poses"], 10, m.edge_ij, m.edge_Z, m.edge_w, 3, **c["params"])
    assert _same_bytes(out[0], c["poses"][0]) and _same_bytes(out[10:], c["poses"][10:])
    assert not _same_bytes(out[1:10], c["poses"][1:10]) and rep[-1] == 9 + 2   # the closure (5, 11) points behind n = 10


def test_skipped_edges_change_nothing():
    c = pg.noisy_case(12, 3, 1)
    clean = pg.log_of(c, cap=8)
    want, wrep = pg.relax(c["poses"], 12, clean.edge_ij, clean.edge_Z, clean.edge_w, 3, **c["params"])
    m = pg.PoseGraphModel(8)
    bad = np.full(12, np.nan)
    m.add([2], c["Z"][0], [1], 14, 100.0, 10.0)        # j >= n
    m.add([c["pairs"][0][0]], c["Z"][0], [1], c["pairs"][0][1], 100.0, 10.0)
    m.edge_ij[m.state[0]] = (3, 3); m.edge_Z[m.state[0]] = c["Z"][0]; m.edge_w[m.state[0]] = (1.0, 1.0); m.state[0] += 1     # i == j
    m.add([c["pairs"][1][0]], c["Z"][1], [1], c["pairs"][1][1], 100.0, 10.0)
    m.edge_ij[m.state[0]] = (1, 5); m.edge_Z[m.state[0]] = bad; m.edge_w[m.state[0]] = (1.0, 1.0); m.state[0] += 1           # a NaN measurement
    m.add([c["pairs"][2][0]], c["Z"][2], [1], c["pairs"][2][1], 100.0, 10.0)
    m.edge_ij[m.state[0]] = (-1, 5); m.edge_Z[m.state[0]] = c["Z"][0]; m.edge_w[m.state[0]] = (1.0, 1.0); m.state[0] += 1    # i < 0
    assert m.state[0] == 7
    got, grep = pg.relax(c["poses"], 12, m.edge_ij, m.edge_Z, m.edge_w, 7, **c["params"])
    assert _same_bytes(got, want) and _same_bytes(grep, wrep)
    # a non-finite pose takes its edges out and passes through unchanged
    poses = c["poses"].copy()
    poses[7, 3] = np.inf
    out, rep = pg.relax(poses, 12, clean.edge_ij, clean.edge_Z, clean.edge_w, 3, **c["params"])
    assert _same_bytes(out[7], poses[7]) and rep[-1] == 9 + 3 and np.isfinite(np.delete(out, 7, 0)).all()


def test_the_consistent_graph_recovers_ground_truth():
    c = pg.consistent_case()
    out, rep = pg.relax_case(c)
    err = np.abs(out - c["gt"]).max()
    print("   consistent graph: cost", rep[:-1].tolist(), "max |pose - truth|", err)
    assert np.abs(c["poses"] - c["gt"]).max() > 0.1    # the input is far from the truth
    assert rep[0] > 1.0 and rep[3] < 1e-12 and rep[-1] == 11 + 17 and err < 1e-12


@pytest.mark.parametrize("n,closures,seed", [(12, 3, 1), (40, 4, 2)])
def test_the_noisy_budgets_are_stationary_and_the_order_of_the_sums_moves_little(n, closures, seed):
    """The budgets the GPU test uses leave the restatement's cost stationary (to 1e-9 relative from the fifth step on), and the restatement differs from
    itself - per-node edge order reversed, dot products pairwise - by no more than the figure the device bound is 100 times of."""
    c = pg.noisy_case(n, closures, seed)
    out, rep = pg.relax_case(c)
    assert abs(rep[4] - rep[10]) < 1e-9 * rep[10] and abs(rep[2] - rep[10]) < 1e-2 * rep[10]
    o2, r2 = pg.relax_case(c, reverse=True, pairwise=True)
    dp, dr = np.abs(out - o2).max(), np.abs(rep - r2).max()
    print("   n", n, "cost", rep[10], "self difference: poses", dp, "report", dr)
    assert dp <= 10 * pg.SELF_POSE[n] and dr <= 10 * pg.SELF_REPORT[n]
