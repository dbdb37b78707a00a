"""Drive sessions (pr_session) without a device: the text of the rule in the header, the ABI surface, the scratch
formula, the argument errors that are returned before any device is touched, what the Python class refuses before it calls the library,
and properties of the NumPy restatement the GPU tests compare the kernels with (session_np.py) - among them the two-drive scene, which
the restatement ALONE must solve with every decision at least 5 % from its threshold, and the 50-digit evaluation of the refinement that
the device bound is derived from.

Measured here (a CPU, NumPy): the scene's G against G_true 1.7e-3 rad and 1.8e-2 m at the closures (bounds 6e-3, 3e-2); largest row
error after align -> gate -> relax across breaks 0.058 m (bound 0.27 m); noise-free 7.1e-15 / 2.3e-14; the restatement's refinement
against 50 digits at most 5.1e-14 over the sweep, so the device bound is at most 5.1e-12 there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gate_np as gn
import posegraph_np as pg
import session_np as sn
from so_dso_place_recognition_amd import _lib, api, graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_session_create", "pr_session_destroy", "pr_session_reset", "pr_session_count", "pr_session_scratch_bytes", "pr_session_begin_dev",
         "pr_session_begin", "pr_session_align_dev", "pr_session_align", "pr_session_relax_dev")


def test_session_header_states_the_rule():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for words in ("pr_session", "DESIGN.md 4.29", "sid(r) = #{q in 1 .. S-1 : start[q] <= r}", "a count, not a search", "BREAK iff sid(r) != sid(r-1)",
                  "S = state[0] clamped into 1 .. session_capacity", "If n == last", "PR_SESSION_REUSED", "until pr_session_reset",
                  "start[S] = n and S + 1 is committed", "info = {session index now current, its first row, S after, flags}",
                  "E = log.state[0] clamped into 0 .. log_edge_capacity", "-1 means S - 1", "PR_SESSION_NO_TARGET",
                  "exactly one end lies in session t and the other in a session < t", "G_a = (P_i^-1 Z_a) P_j", "G_a = (P_j^-1 Z_a^-1) P_i",
                  "c_a = -(R^T t)", "q_a != q_b", "c_rot = 3 - ((x00 + x11) + x22) <= rot_c_max", "d = G_a c_b - G_b c_b",
                  "AT THE CLOSURE, not at the world origin", "A NaN supports nothing", "ties to the lowest log index", "PR_SESSION_NO_CANDIDATE",
                  "support + 1 < min_inliers: PR_SESSION_WEAK", "R = R_Ga* exp(mean_b log_SO3(R_Ga*^T R_Gb))", "t = mean_b(G_b c_b) - R mean_b(c_b)",
                  "PR_SESSION_NONFINITE", "becomes P_r G^-1", "rows >= n are not written", "info = {status, a* or -1, its support, candidates, |I|, E, n, flags}",
                  "odometry slot s is not an edge when row s + 1 is a break", "exactly pr_posegraph_relax_dev's bytes", "Node 0 remains the only gauge",
                  "3 outer + 4 launches in all", "4 launches (prepare, pairs, choose, apply)", "(a0 b0 + a1 b1) + a2 b2", "+Inf is allowed",
                  "4 NC (sid) | 4 NC (breaks) | 4 EC (candidate) | 4 EC (q) | 96 EC (G_a) | 24 EC (c_a) | 24 EC (G_a c_a)"):
        assert words in txt, words
    doc = sn.__doc__
    for words in ("exactly one end in t", "G_a = (P_i^-1 Z_a) P_j", "ties to the lowest index", "P_r G^-1"):
        assert words in doc, words


def test_session_symbols_records_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_session_")) == sorted(NAMES)
    assert "typedef struct pr_session_buffers { int32_t* start; int32_t* state; } pr_session_buffers;" in code
    assert "typedef struct pr_session_align_params { int32_t session, min_inliers; double rot_c_max, trans2_max; } pr_session_align_params;" in code
    assert C.sizeof(_lib.SessionAlignParams) == 24 and C.sizeof(_lib.SessionBuffers) == 2 * C.sizeof(C.c_void_p)
    assert "#define PR_SESSION_OVERFLOW 1" in code and "#define PR_SESSION_REUSED 2" in code and "#define PR_SESSION_LOG_OVERFLOW 4" in code
    assert (_lib.SESSION_OVERFLOW, _lib.SESSION_REUSED, _lib.SESSION_LOG_OVERFLOW) == (sn.OVERFLOW, sn.REUSED, sn.LOG_OVERFLOW) == (1, 2, 4)
    for k, name in enumerate(("ALIGNED", "NO_TARGET", "NO_CANDIDATE", "WEAK", "NONFINITE")):
        assert re.search(r"PR_SESSION_%s = %d\b" % (name, k), code) and getattr(_lib, "SESSION_" + name) == k == getattr(sn, name)
    for m in ("begin_torch", "begin_map", "begin", "align_torch", "align_map", "align", "relax_torch", "relax_map", "count", "reset",
              "scratch_bytes", "close"):
        assert hasattr(graph.SessionTable, m), m
    from so_dso_place_recognition_amd._handle import Handle
    assert issubclass(graph.SessionTable, Handle) and issubclass(api.ClosureGate, Handle)      # the shared base
    assert graph.SessionAlign._fields == ("poses", "G", "hyp", "support", "inlier", "info")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"session\.o: session\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "session_host.o" in mk
    hip = open(os.path.join(CSRC, "session.hip")).read()
    assert "atomicAdd(&v.sup[a], count)" in hip and hip.count("atomicAdd(") == 1          # the one atomic: an integer counter
    pgh = open(os.path.join(CSRC, "posegraph.hip")).read()
    assert "!(brk && brk[s + 1])" in pgh                                                   # NULL leaves the odometry rule as it was


def test_session_scratch_size_formula():
    lib = _lib.load()
    for nc, ec, sc in ((40, 600, 4), (1, 1, 1), (1 << 20, 65536, 1024), (16, 8, 2), (3475, 173, 40), (44, 257, 5), (80, 16, 4)):
        want = sn.scratch_bytes(nc, ec, sc)
        assert want > 8 * nc + 257 * ec and lib.pr_session_scratch_bytes(nc, ec, sc) == want, (nc, ec, sc)
    for bad in ((0, 1, 1), ((1 << 20) + 1, 1, 1), (8, 0, 1), (8, 65537, 1), (8, 1, 0), (8, 1, 1025)):
        assert lib.pr_session_scratch_bytes(*bad) == 0 == sn.scratch_bytes(*bad), bad


def test_session_argument_errors_before_any_device():
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    store = (C.c_double * 16)()
    base = C.addressof(store)
    rec = lambda: _lib.SessionBuffers(base, base + 8)

    def create(b=True, nc=8, ec=4, sc=2, out=True):
        h = C.c_void_p(1)
        r = b if isinstance(b, _lib.SessionBuffers) else (rec() if b else None)
        rc = lib.pr_session_create(None, C.byref(r) if r is not None else None, nc, ec, sc, C.byref(h) if out else None)
        assert rc == _lib.PR_EINVAL and (not out or not h.value)
        return err()

    assert "out is NULL" in create(out=False) and "buffers is NULL" in create(b=None)
    for name in ("start", "state"):
        r = rec(); setattr(r, name, None)
        assert "a buffer is NULL" in create(b=r), name
    for nc in (0, -1, (1 << 20) + 1):
        assert "node_capacity=%d outside" % nc in create(nc=nc)
    for ec in (0, -1, 65537):
        assert "edge_capacity=%d outside" % ec in create(ec=ec)
    for sc in (0, -1, 1025):
        assert "session_capacity=%d outside" % sc in create(sc=sc)
    assert "ctx is NULL" in create(nc=1 << 20, ec=65536, sc=1024)     # the last check: everything else was in order
    buf = (C.c_double * 16)()
    e = lambda: lib.pr_last_error(None)
    assert lib.pr_session_reset(None) == _lib.PR_EINVAL and b"pr_session_reset: session table is NULL" in e()
    w = C.c_int32()
    assert lib.pr_session_count(None, C.byref(w), C.byref(w)) == _lib.PR_EINVAL and b"pr_session_count: session table is NULL" in e()
    assert lib.pr_session_begin_dev(None, buf, buf) == _lib.PR_EINVAL and b"pr_session_begin_dev: session table is NULL" in e()
    assert lib.pr_session_begin(None, buf, buf) == _lib.PR_EINVAL and b"pr_session_begin: session table is NULL" in e()
    lib.pr_session_destroy(None)                        # a no-op
    log = _lib.PoseGraphBuffers(base, base + 8, base + 16, base + 24)
    for fn in ("pr_session_align_dev", "pr_session_align"):
        def al(prm=(-1, 3, 0.1, 1.0), lg=log):
            p = _lib.SessionAlignParams(*prm) if prm is not None else None
            rc = getattr(lib, fn)(None, C.byref(lg) if lg is not None else None, 4, buf, buf, C.byref(p) if p is not None else None, buf, buf,
                                  None, None, None, buf)
            assert rc == _lib.PR_EINVAL
            return err()
        assert fn + ": params is NULL" in al(prm=None)
        assert "session=-2 is below -1" in al(prm=(-2, 3, 0.1, 1.0)) and "min_inliers=0 is below 1" in al(prm=(-1, 0, 0.1, 1.0))
        for bad in (float("nan"), -1e-300, -float("inf")):
            assert "rot_c_max is NaN or negative" in al(prm=(-1, 3, bad, 1.0)) and "trans2_max is NaN or negative" in al(prm=(-1, 3, 0.1, bad))
        assert "buffer record is NULL" in al(lg=None)
        for name in api.PoseGraph.NAMES:
            lg = _lib.PoseGraphBuffers(base, base + 8, base + 16, base + 24); setattr(lg, name, None)
            assert "a buffer of the log is NULL" in al(lg=lg), name
        assert fn + ": session table is NULL" in al(prm=(-1, 1, float("inf"), 0.0))         # +Inf and 0 are allowed
    prm = _lib.PoseGraphParams(1, 1, 0.0, 1.0, 1.0)
    assert lib.pr_session_relax_dev(None, None, buf, buf, None, buf, buf) == _lib.PR_EINVAL and b"pr_session_relax_dev: params is NULL" in e()
    bad = _lib.PoseGraphParams(0, 1, 0.0, 1.0, 1.0)
    assert lib.pr_session_relax_dev(None, None, buf, buf, C.byref(bad), buf, buf) == _lib.PR_EINVAL and b"pr_session_relax_dev: outer=0" in e()
    assert lib.pr_session_relax_dev(None, None, buf, buf, C.byref(prm), buf, buf) == _lib.PR_EINVAL and b"pr_session_relax_dev: graph is NULL" in e()


def test_session_table_refuses_before_the_library():
    import torch

    class Fake:
        NAMES = api.PoseGraph.NAMES
    ctx = Fake(); ctx.lib = None
    s = graph.SessionTable.__new__(graph.SessionTable)  # no handle, no library call: the checks are the first thing a method does
    s.ctx, s.h, s.node_capacity, s.edge_capacity, s.session_capacity = ctx, None, 8, 4, 2
    pgf = Fake(); pgf.ctx, pgf.node_capacity, pgf.edge_capacity = ctx, 8, 4
    cpu = torch.zeros((8, 12), dtype=torch.float64)
    n = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="n must be a contiguous CUDA tensor"):
        s.begin_torch(n)
    with pytest.raises(ValueError, match="n must be"):
        s.begin(n)
    with pytest.raises(ValueError, match="poses must be a contiguous CUDA tensor"):
        s.align_torch(pgf, cpu, n)
    with pytest.raises(ValueError, match="poses must be"):
        s.align(pgf, cpu, n)
    with pytest.raises(ValueError, match="poses must be"):
        s.relax_torch(pgf, cpu, n)
    pgf.edge_capacity = 5
    with pytest.raises(ValueError, match="must not exceed the session table's"):
        s.align_torch(pgf, cpu, n)
    pgf.edge_capacity, pgf.node_capacity = 4, 9
    with pytest.raises(ValueError, match="node_capacity must equal the session table's"):
        s.relax_torch(pgf, cpu, n)
    pgf.ctx = object()
    for call in (lambda: s.align_torch(pgf, cpu, n), lambda: s.relax_torch(pgf, cpu, n)):
        with pytest.raises(ValueError, match="share one context"):
            call()
    km = Fake(); km.ctx, km.keyframe_capacity = object(), 8
    for call in (lambda: s.begin_map(km), lambda: s.align_map(km, pgf), lambda: s.relax_map(km, pgf)):
        with pytest.raises(ValueError, match="share one context"):
            call()
    km.ctx, km.keyframe_capacity = ctx, 9
    with pytest.raises(ValueError, match="keyframe_capacity"):
        s.begin_map(km)


# ------------------------------------------------------------------------------------------------ the restatement: the table
def test_sid_under_monotone_and_scribbled_starts():
    m = sn.SessionModel(40, 5)
    for s in (8, 16, 24):
        m.begin(s)
    assert m.sid(np.arange(40)).tolist() == [0] * 8 + [1] * 8 + [2] * 8 + [3] * 16 and np.flatnonzero(m.breaks(40)).tolist() == [8, 16, 24]
    m.start[:] = (99, 30, -5, 30, 7)                    # scribbled: start[0] is never read, the count is defined all the same
    m.state[0] = 1 << 30                                # clamped to the capacity: all five entries count
    want = [sum(1 for q in (30, -5, 30, 7) if q <= r) for r in range(40)]
    assert m.S == 5 and m.sid(np.arange(40)).tolist() == want and want[0] == 1 and want[7] == 2 and want[30] == 4
    assert np.flatnonzero(m.breaks(40)).tolist() == [7, 30]
    m.state[0] = -3
    assert m.S == 1 and not m.sid(np.arange(40)).any() and not m.breaks(40).any()       # S = 1 breaks nothing


def test_the_begin_rule_reuse_overflow_and_n_zero():
    m = sn.SessionModel(40, 3)
    assert m.begin(0).tolist() == [0, 0, 1, sn.REUSED] and m.state.tolist() == [1, 0, 0, 0]          # n = 0: session 0 is still empty
    assert m.begin(12).tolist() == [1, 12, 2, 0] and m.begin(12).tolist() == [1, 12, 2, sn.REUSED]
    assert m.begin(99).tolist() == [2, 40, 3, 0]                                                    # n is clamped to the node capacity
    assert m.begin(40).tolist() == [2, 40, 3, sn.REUSED] and m.state[1] == 0                         # reuse comes before overflow
    assert m.begin(30).tolist() == [2, 40, 3, sn.OVERFLOW] and m.state.tolist() == [3, sn.OVERFLOW, 0, 0] and m.start.tolist() == [0, 12, 40]
    assert m.begin(40).tolist() == [2, 40, 3, sn.OVERFLOW | sn.REUSED]                               # it stays set in every later info
    m.reset()
    assert m.state.tolist() == [1, 0, 0, 0] and m.begin(5).tolist() == [1, 5, 2, 0]


# ------------------------------------------------------------------------------------------------ the restatement: the alignment
def test_both_orientations_give_the_planted_transform_on_noise_free_data():
    gt = pg.circle_truth(44, 2, radius=20.0)
    poses = sn.drives(gt, [0, 20], 40, 0, None)
    model = sn.SessionModel(44, 2); model.begin(20)
    Zf = lambda i, j: pg.measure(gt, i, j)
    edges = [(3, 25, Zf(3, 25), sn.W), (31, 7, Zf(31, 7), sn.W), (12, 38, Zf(12, 38), sn.W), (22, 0, Zf(22, 0), sn.W)]
    r = sn.align(model, poses, 40, sn._log(edges, 8), 8)
    assert r["info"].tolist() == [sn.ALIGNED, 0, 3, 4, 4, 4, 40, 0] and r["support"][:4].tolist() == [3] * 4
    assert np.abs(r["hyp"][:4].reshape(4, 3, 4) - sn.frame(1)).max() < 1e-12 and np.abs(r["G"].reshape(3, 4) - sn.frame(1)).max() < 1e-12
    assert np.abs(r["poses"][:40] - gt[:40]).max() < 1e-12 and r["poses"][:20].tobytes() == poses[:20].tobytes()


def test_support_is_invariant_under_a_common_rigid_motion_of_the_target():
    c = sn.sweep_case(65)
    r = sn.run_case(c, margins=True)
    M = np.concatenate([pg.exp_so3(np.array([0.7, -1.1, 0.4])), np.array([[-12.0], [50.0], [3.0]])], axis=1)
    moved = c["poses"].copy()
    moved[20:40] = pg.mul(pg.as34(c["poses"][20:40]), M).reshape(20, 12)
    r2 = sn.run_case(dict(c, poses=moved), margins=True)
    assert r["margin"] > 1e-6 and r2["margin"] > 1e-6
    for k in ("support", "inlier", "info"):
        assert np.array_equal(r[k], r2[k]), k
    assert np.abs(r["poses"][:40] - r2["poses"][:40]).max() < 1e-10     # the aligned rows do not depend on the frame the drive came in


def test_ties_go_to_the_lowest_log_index():
    gt = pg.circle_truth(44, 2, radius=20.0)
    poses = sn.drives(gt, [0, 20], 40, 0, None)
    model = sn.SessionModel(44, 2); model.begin(20)
    Zf = lambda i, j: pg.measure(gt, i, j)
    Gs = sn.frame(1).copy(); Gs[0, 3] += 9.0                         # a second consensus: the same frame shifted by 9 m
    shifted = lambda i, j: pg.mul(pg.mul(pg.as34(gt[i]), Gs), pg.inv(pg.as34(poses[j]))).reshape(12)
    edges = [(1, 2, Zf(1, 2), sn.W), (5, 30, shifted(5, 30), sn.W), (6, 31, shifted(6, 31), sn.W), (3, 25, Zf(3, 25), sn.W), (4, 26, Zf(4, 26), sn.W)]
    r = sn.align(model, poses, 40, sn._log(edges, 8), 8, min_inliers=2)
    assert r["support"][:5].tolist() == [-1, 1, 1, 1, 1] and r["info"][:5].tolist() == [sn.ALIGNED, 1, 1, 4, 2] and r["inlier"][:5].tolist() == [0, 1, 1, 0, 0]


def test_statuses_without_an_alignment_copy_the_poses():
    c = sn.sweep_case(65, S=3, target=1)
    for kw, status in ((dict(session=0), sn.NO_TARGET), (dict(session=3), sn.NO_TARGET), (dict(min_inliers=60), sn.WEAK)):
        r = sn.run_case(c, **kw)
        assert r["info"][0] == status and r["poses"].tobytes() == c["poses"].tobytes() and r["G"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], kw
    one = sn.sweep_case(9, S=3, target=1, one_q=True)
    assert sn.run_case(one, min_inliers=2)["info"][:5].tolist() == [sn.WEAK, 0, 0, 9, 1]
    assert sn.run_case(one, min_inliers=1)["info"][:5].tolist() == [sn.ALIGNED, 0, 0, 9, 1]
    empty = sn.sweep_case(0)
    assert sn.run_case(empty)["info"].tolist() == [sn.NO_CANDIDATE, -1, 0, 0, 0, 3, 40, 0]
    assert sn.run_case(dict(empty, n=20))["info"][0] == sn.NO_TARGET                     # session 1 has no row below n


def test_the_tie_across_strides_the_overflowing_sum_and_the_many_row_case():
    r = sn.run_case(sn.tie_case(), margins=True)
    assert r["info"].tolist() == [sn.ALIGNED, 300, 1, 4, 2, 515, 40, 0] and np.flatnonzero(r["inlier"]).tolist() == [300, 301]
    assert r["support"][[300, 301, 513, 514]].tolist() == [1, 1, 1, 1] and r["margin"] > 0.5
    c = sn.nonfinite_case()
    r = sn.run_case(c)
    assert r["info"].tolist() == [sn.NONFINITE, 0, 1, 2, 2, 2, 16, 0] and np.isfinite(r["hyp"]).all() and r["poses"].tobytes() == c["poses"].tobytes()
    assert r["G"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and r["inlier"][:2].tolist() == [1, 1]
    big = sn.sweep_case(65, rows=(600, 580), starts=[0, 300])
    r = sn.run_case(big, margins=True, exact=True)
    assert r["info"][0] == sn.ALIGNED and r["info"][3] == 65 and r["margin"] >= 1e-6 and r["rows"].tolist() == list(range(300, 580))


@pytest.mark.parametrize("name", sorted(sn.exact_cases()))
def test_thresholds_in_exact_arithmetic(name):
    c, want = sn.exact_cases()[name]
    r = sn.run_case(c)
    assert r["support"][:2].tolist() == want and r["info"][0] == sn.ALIGNED
    assert np.array_equal(r["hyp"][0].reshape(3, 4), c["Gt"]) or name.startswith("flipped")          # the lattice is exact


@pytest.mark.parametrize("C", [c for c in sn.SWEEP_CANDIDATES if c >= 2])
def test_no_decision_of_a_sweep_case_hangs_on_a_rounding(C):
    r = sn.run_case(sn.sweep_case(C), margins=True)
    assert r["margin"] >= 1e-6 and r["info"][3] == C


def test_the_refinement_matches_a_50_digit_evaluation():
    """the difference measured here, times MARGIN, is the bound the GPU test uses for G and the moved rows (session_np.device_bound)"""
    worst = 0.0
    for c in (sn.sweep_case(65), sn.sweep_case(513), sn.scene()):
        r = sn.run_case(c, exact=True)
        dG = float(np.abs(r["G"] - r["G_mp"]).max())
        dP = float(np.abs(r["poses"] - r["poses_mp"]).max())
        bG, bP = sn.device_bound(r)
        print(f"   |I| {r['info'][4]}: |G - G_50| {dG:.2e} |rows - rows_50| {dP:.2e} -> device bounds {bG:.2e} {bP:.2e}")
        assert dG <= 64 * sn.EPS * 64.0 and dP <= 64 * sn.EPS * 64.0     # a few roundings of entries below 64
        assert bG >= sn.MARGIN * sn.EPS and bP >= sn.MARGIN * sn.EPS
        worst = max(worst, dG, dP)
    assert worst < 1e-12


def test_the_break_rule_drops_exactly_the_border_slots():
    c = sn.scene()
    lg = c["log"]
    args = (c["poses"], 80, lg.edge_ij, lg.edge_Z, lg.edge_w, 12, 100.0, 10.0)
    I0, J0, Z0, W0, l0 = pg.used_edges(*args)
    I1, J1, Z1, W1, l1 = sn.used_edges(c["model"], *args)
    gone = [(i, j) for i, j in zip(I0.tolist(), J0.tolist()) if (i, j) not in set(zip(I1.tolist(), J1.tolist()))]
    assert gone == [(39, 40)] and l0 == l1 == 12 and len(I1) == len(I0) - 1
    one = sn.SessionModel(80, 4)                        # S = 1 breaks nothing
    I2, J2, Z2, W2, l2 = sn.used_edges(one, *args)
    assert np.array_equal(I2, I0) and np.array_equal(J2, J0) and Z2.tobytes() == Z0.tobytes()
    a, ra = pg.relax(c["poses"], 80, lg.edge_ij, lg.edge_Z, lg.edge_w, 12, **sn.SCENE_RELAX)
    b, rb = sn.relax(one, c["poses"], 80, lg.edge_ij, lg.edge_Z, lg.edge_w, 12, **sn.SCENE_RELAX)
    assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes() and pg.used_edges.__module__ == "posegraph_np"


# ------------------------------------------------------------------------------------------------ the two-drive scene
def test_the_restatement_alone_joins_the_two_drives():
    c = sn.scene()
    a, g, dst, out, rep = sn.scene_chain(c)
    assert a["info"].tolist() == [sn.ALIGNED, 0, 8, 12, 9, 12, 80, 0]
    assert np.flatnonzero(a["inlier"]).tolist() == c["true_rows"]                        # exactly the nine true closures
    assert a["margin"] >= 0.05                                                           # every decision at least 5 % from its threshold
    G, Gt = a["G"].reshape(3, 4), c["Gt"]
    ang = float(np.linalg.norm(pg.log_so3(gn.rmul(gn.rinv(Gt), G)[:, :3])[0]))
    q = np.array([j for (i, j) in c["log"].edge_ij[c["true_rows"]]])
    cm = sn.centres(c["poses"][q]).mean(0)
    dt = float(np.linalg.norm((gn.mv3(G[:, :3], cm) + G[:, 3]) - (gn.mv3(Gt[:, :3], cm) + Gt[:, 3])))
    e_in = np.linalg.norm(sn.centres(c["poses"]) - sn.centres(c["gt"]), axis=1)
    e_al = np.linalg.norm(sn.centres(a["poses"]) - sn.centres(c["gt"]), axis=1)
    e_rl = np.linalg.norm(sn.centres(out) - sn.centres(c["gt"]), axis=1)
    print(f"   scene: G against G_true {ang:.2e} rad (bound {sn.SCENE_G_ROT:.0e}) {dt:.2e} m at the closures (bound {sn.SCENE_G_TRANS:.0e}); margin "
          f"{a['margin']:.3f}; row error input {e_in.max():.1f} aligned {e_al.max():.3f} relaxed {e_rl.max():.3f} (bound {sn.SCENE_ROW_BOUND:.2f}); "
          f"gate {g['info'].tolist()} margin {g['margin']:.2e}; cost {rep[0]:.3e} -> {rep[-2]:.3e}, edges {rep[-1]:.0f}")
    assert ang <= sn.SCENE_G_ROT and dt <= sn.SCENE_G_TRANS
    assert g["info"].tolist() == [12, 9, 12, 0] and np.flatnonzero(g["keep"]).tolist() == c["true_rows"] and g["margin"] >= 1e-6
    assert e_in[40:].min() > 10.0 and e_rl.max() <= sn.SCENE_ROW_BOUND and rep[-1] == 78 + 9 and rep[-2] < rep[0]
    assert out[0].tobytes() == c["poses"][0].tobytes()                                   # node 0 is the only gauge


def test_the_noise_free_scene_recovers_the_truth_to_rounding():
    c = sn.scene(noise=False)
    r = sn.run_case(c)
    assert r["info"][:5].tolist() == [sn.ALIGNED, 0, 8, 12, 9]
    dG, dP = float(np.abs(r["G"].reshape(3, 4) - c["Gt"]).max()), float(np.abs(r["poses"] - c["gt"]).max())
    print(f"   noise-free scene: |G - G_true| {dG:.2e} |rows - truth| {dP:.2e}")
    assert dG <= 1e-9 and dP <= 1e-9                                                     # rounding only, eight orders below the misalignment
    assert np.abs(c["poses"][40:] - c["gt"][40:]).max() > 10.0
