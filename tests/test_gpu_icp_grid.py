"""The exact uniform-grid correspondence search on the device (csrc/icp_grid.hip).  pr_icp_nn_radius in GRID mode against
BRUTE mode on the device and against the restatement icp_grid_np.py (= icp_np.py masked to d2 < max_corr^2) on the host: every
comparison is torch.equal on the indices and on d2 viewed as int64.  Refinement: with GRID, pr_icp_pairs_dev returns the bytes BRUTE
returns under pr_set_icp_path(ctx, 2) - the same chunks of 256 source points, the same sums by the same code -, and relates to the other
geometries and to the restatement as the split path does: status, iters, n_inl, fitness equal, rmse, R, t within the 1e-10 of
test_gpu_icp.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import icp_cases
import icp_grid_np
import icp_np
from so_dso_place_recognition_amd import _lib, api

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")
TOL = 1e-10
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def same(idx_a, d2_a, idx_b, d2_b):
    ia, ib = torch.from_numpy(np.ascontiguousarray(idx_a, np.int32)), torch.from_numpy(np.ascontiguousarray(idx_b, np.int32))
    da, db = torch.from_numpy(np.ascontiguousarray(d2_a, np.float64)), torch.from_numpy(np.ascontiguousarray(d2_b, np.float64))
    return torch.equal(ia, ib) and torch.equal(da.view(torch.int64), db.view(torch.int64))


def rigid(deg, t, axis=(0.3, -0.8, 0.5)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.hstack([np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K, np.asarray(t, np.float64)[:, None]])


def restated(clouds_q, clouds_d, pairs, T, mc, ms=None, md=None):
    offs, wi, wd = [0], [], []
    for (s, d), Ti in zip(pairs, T):
        if s < 0 or d < 0:
            offs.append(offs[-1]); continue
        j, v = icp_grid_np.nn_radius(icp_np.transform(Ti, clouds_q[s][:ms]), clouds_d[d][:md], mc)
        wi.append(j); wd.append(v); offs.append(offs[-1] + len(j))
    return np.array(offs), (np.concatenate(wi) if wi else np.zeros(0, np.int32)), (np.concatenate(wd) if wd else np.zeros(0))


def radius_both(ctx, clouds_q, clouds_d, pairs, T, mc):
    """pr_icp_nn_radius in both search modes, each equal to the restatement (hence to each other) bit for bit; returns (offs, idx, d2)."""
    xq, oq = icp_cases.csr(clouds_q)
    xd, od = icp_cases.csr(clouds_d)
    ps = np.array([p[0] for p in pairs], np.int32); pd = np.array([p[1] for p in pairs], np.int32)
    offs, wi, wd = restated(clouds_q, clouds_d, pairs, T, mc)
    got = {}
    for search in ("brute", "grid"):
        before = ctx.lib.pr_get_icp_search(ctx.h)
        go, gi, gd = api.icp_nn_radius(xq, oq, xd, od, ps, pd, np.asarray(T), mc, ctx=ctx, search=search)
        assert ctx.lib.pr_get_icp_search(ctx.h) == before
        assert np.array_equal(go, offs), (search, go, offs)
        assert same(gi, gd, wi, wd), (search, np.flatnonzero((gi != wi) | (gd.view(np.int64) != wd.view(np.int64)))[:8])
        got[search] = (gi, gd)
    assert same(*got["grid"], *got["brute"])
    return offs, wi, wd


# ------------------------------------------------------------------------------------------ 1. random boxes
def test_random_boxes_sizes_shared_clouds_and_missing_pairs(ctx):
    rng = np.random.default_rng(21)
    src_sizes = (0, 1, 63, 64, 65, 257)
    dst_sizes = (0, 1, 255, 256, 257, 515)
    # a box of side L holds n points: a ball of radius 1 holds n (4/3 pi) / L^3 of them; about 0.7 on average -> half the sources have one
    cd = [rng.random((n, 3)) * (max(n, 1) * 4.19 / 0.7) ** (1 / 3) for n in dst_sizes]
    cq = [rng.random((n, 3)) * (515 * 4.19 / 0.7) ** (1 / 3) for n in src_sizes]
    pairs = [(s, d) for s in range(len(cq)) for d in range(len(cd))]                  # every source and every target in several pairs
    pairs += [(-1, 2), (3, -1), (-1, -1), (5, 5)]
    T = [IDENT if i % 3 == 0 else rigid(3.0 * (i % 5) + 1, rng.normal(0, 0.5, 3)) for i in range(len(pairs))]
    offs, wi, wd = radius_both(ctx, cq, cd, pairs, T, 1.0)
    assert offs[-1] == sum(src_sizes) * len(dst_sizes) + 257
    i = pairs.index((5, 5))
    frac = (wi[offs[i]:offs[i + 1]] >= 0).mean()
    print("   sources with a neighbour inside max_corr, 257 x 515:", frac)
    assert 0.25 < frac < 0.75
    for i, (s, d) in enumerate(pairs):
        if d == 0 and s >= 0:                                                        # an empty target: no correspondents anywhere
            assert np.all(wi[offs[i]:offs[i + 1]] == -1) and np.all(np.isinf(wd[offs[i]:offs[i + 1]]))


# ------------------------------------------------------------------------------------------ 2. integer lattices, max_corr = 1
def test_lattice_borders_strict_radius_ties_and_duplicates(ctx):
    rng = np.random.default_rng(22)
    g = np.arange(5.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    dst = np.concatenate([lat, lat[[7, 7, 62, 124, 0]]])                              # duplicates of single target points
    dst = dst[rng.permutation(len(dst))]
    cells, G = icp_grid_np.plan(1, len(dst))
    h = float(icp_grid_np.cell_edge(1.0, 4.0, G))
    assert h == 1.0 * icp_grid_np.SLACK                                               # max_corr sets the cell edge here
    one = np.nextafter(1.0, 0.0)
    assert one == 1.0 - 2.0 ** -53
    src = []
    yz = [(0.0, 0.0), (2.0, 3.0), (4.0, 4.0), (1.0, 2.0)]
    for a in range(3):
        for u, v in yz:
            for x in (-1.0, 5.0,                                                      # exactly 1.0 from the face: not an inlier (strict)
                      -(1.0 - 2.0 ** -52), np.nextafter(5.0, 0.0), -one, np.nextafter(np.nextafter(5.0, 0.0), 0.0),   # just inside, one cell outside the box
                      0.5, 1.5, 2.5, 3.5):                                            # exact ties between two lattice points
                p = [u, v]; p.insert(a, x); src.append(p)
            for kcell in range(1, 4):                                                 # on a cell border and one ulp either side of it
                b = kcell * h
                for x in (b, np.nextafter(b, 0.0), np.nextafter(b, 9.0)):
                    p = [u + 0.25, v - 0.25]; p.insert(a, x); src.append(p)
    a_ = 0.577
    for sx in (-a_, 4 + a_):                                                          # diagonal neighbours across cell corners
        for sy in (-a_, 4 + a_):
            for sz in (-a_, 4 + a_):
                src.append([sx, sy, sz])
    src += [[-0.6, -0.6, -0.6], [1.5, 1.5, 1.5], [1.5, 2.5, 0.5], [2.0, 2.0, 2.0], [0.0, 0.0, 1.0]]     # outside corner; 8- and 4-fold ties; duplicates
    src = np.array(src, np.float64)
    offs, wi, wd = radius_both(ctx, [src], [dst], [(0, 0)], [IDENT], 1.0)
    first = {tuple(q): j for j, q in reversed(list(enumerate(dst)))}
    exact_one = [i for i, p in enumerate(src) if np.sum((p == -1.0) | (p == 5.0)) == 1 and np.all(p == np.round(p))]
    assert len(exact_one) == 24 and np.all(wi[exact_one] == -1) and np.all(np.isinf(wd[exact_one]))
    inside = [i for i, p in enumerate(src) if np.any((np.abs(p) == 1.0 - 2.0 ** -52) | (np.abs(p) == one) | (p == np.nextafter(5.0, 0.0)) | (p == np.nextafter(np.nextafter(5.0, 0.0), 0.0)))]
    assert len(inside) == 48 and np.all(wi[inside] >= 0) and np.all(wd[inside] < 1.0) and np.all(wd[inside] > 1.0 - 1e-14)
    for i, p in enumerate(src):                                                       # ties: the smallest index among the equidistant lattice points
        if np.all((p >= 0) & (p <= 4)) and np.all(p * 2 == np.round(p * 2)):
            lo, hi = np.floor(p), np.ceil(p)
            cands = [first[(x, y, z)] for x in {lo[0], hi[0]} for y in {lo[1], hi[1]} for z in {lo[2], hi[2]}]
            assert wi[i] == min(cands), (p, wi[i], cands)
    assert wi[len(src) - 5] == -1                                                     # (-0.6, -0.6, -0.6): d2 = 1.08
    corners = slice(len(src) - 13, len(src) - 5)
    assert np.all(wi[corners] >= 0) and np.all(wd[corners] < 1.0)


# ------------------------------------------------------------------------------------------ 3. non-finite and extreme values
def test_non_finite_coordinates_far_sources_and_degenerate_boxes(ctx):
    rng = np.random.default_rng(23)
    src = rng.random((140, 3)) * 8; dst = rng.random((300, 3)) * 8
    src[5, 1] = np.nan; src[6, 0] = np.inf; src[7] = -np.inf; src[8] = [1e300, 2.0, 2.0]; src[9] = [-1e300, 1e300, 1e300]; src[10] = [30.0, 4.0, 4.0]
    dst[0, 2] = np.nan; dst[3, 0] = np.inf; dst[256, 1] = -np.inf; dst[257] = np.nan
    all_bad = np.full((9, 3), np.nan); all_bad[::2] = np.inf
    far = dst.copy(); far[100] = [1e6, -1e6, 1e6]                                     # one finite point inflates the box: h far above max_corr
    same_pt = np.tile([[1.5, -2.25, 3.0]], (70, 1))                                   # a target of coincident points: one cell
    near_same = np.tile([[1.5, -2.25, 3.0]], (40, 1)) + rng.normal(0, 0.5, (40, 3))
    near_same[0] = [1.5, -2.25, 3.0]
    pairs = [(0, 0), (1, 1), (0, 1), (0, 2), (2, 3)]
    T = [rigid(4, (0.2, -0.1, 0.1)), IDENT, IDENT, IDENT, IDENT]
    offs, wi, wd = radius_both(ctx, [src, src[:20], near_same], [dst, all_bad, far, same_pt], pairs, T, 1.0)
    assert np.all(wi[5:10] == -1) and np.all(np.isinf(wd[5:10]))
    assert not np.isin(wi[:140], (0, 3, 256, 257)).any()
    assert np.all(wi[140:300] == -1)                                                  # an all-non-finite target
    w = wi[offs[4]:offs[5]]
    assert w[0] == 0 and (w >= 0).any() and (w < 0).any() and set(w.tolist()) <= {-1, 0}      # coincident points: the first one answers
    cloud = (rng.random((3000, 3)) - 0.5) * [50.0, 4.0, 50.0]                         # max_corr = 1e-3 on a 50 m cloud: the budget sets h
    probe = np.concatenate([cloud[:200] + rng.normal(0, 4e-4, (200, 3)), cloud[200:260] + 2e-3])
    cells, G = icp_grid_np.plan(1, 3000)
    assert 50.0 / G > 1.0                                                             # metres per cell, three orders above max_corr
    offs, wi, wd = radius_both(ctx, [probe], [cloud], [(0, 0)], [IDENT], 1e-3)
    assert 100 < (wi >= 0).sum() <= 200 and np.all(wi[200:] == -1)


def radius_dev(ctx, xq, oq, xd, od, ps, pd, T, ms, md, mc, search):
    c = len(ps)
    t = [dev(xq), dev(oq, np.int64), dev(xd), dev(od, np.int64), dev(ps, np.int32), dev(pd, np.int32), dev(T)]
    total = int(sum(min(oq[s + 1] - oq[s], ms) for s, d in zip(ps, pd) if s >= 0 and d >= 0))
    oo = torch.zeros(c + 1, dtype=torch.int64, device="cuda"); nj = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    nd = torch.zeros(max(total, 1), dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    torch.cuda.synchronize()
    with api.icp_search(ctx, search):
        ctx.check(ctx.lib.pr_icp_nn_radius_dev(ctx.h, p(t[0]), p(t[1]), len(oq) - 1, p(t[2]), p(t[3]), len(od) - 1, p(t[4]), p(t[5]), c, p(t[6]),
                                               ms, md, mc, p(oo), p(nj), p(nd)))
        ctx.check(ctx.lib.pr_sync(ctx.h))
    return oo.cpu().numpy(), nj.cpu().numpy()[:total], nd.cpu().numpy()[:total]


def test_clouds_are_read_up_to_the_bounds_of_the_call(ctx):
    rng = np.random.default_rng(24)
    cq = [rng.random((90, 3)) * 6, rng.random((40, 3)) * 6]; cd = [rng.random((400, 3)) * 6, rng.random((100, 3)) * 6]
    pairs = [(0, 0), (1, 1), (0, 1)]
    T = [IDENT, rigid(5, (0.1, 0.1, 0.0)), IDENT]
    xq, oq = icp_cases.csr(cq); xd, od = icp_cases.csr(cd)
    ps = np.array([p[0] for p in pairs], np.int32); pd = np.array([p[1] for p in pairs], np.int32)
    for ms, md in ((90, 400), (64, 130), (1, 1), (90, 0)):
        offs, wi, wd = restated(cq, cd, pairs, T, 1.0, ms, md)
        for search in ("brute", "grid"):
            go, gi, gd = radius_dev(ctx, xq, oq, xd, od, ps, pd, np.stack(T), ms, md, 1.0, search)
            assert np.array_equal(go, offs) and same(gi, gd, wi, wd), (ms, md, search)
    assert (wi >= 0).sum() == 0 and len(wi) == 220                                    # max_dst_pts = 0: nothing to find


# ------------------------------------------------------------------------------------------ 4. refinement
def refine(ctx, name, search, path=0, **over):
    c = icp_cases.case(name)
    xq, oq = icp_cases.csr([c["P"]]); xd, od = icp_cases.csr([c["Q"]])
    prm = dict(icp_cases.PARAMS); prm.update(over)
    ctx.check(ctx.lib.pr_set_icp_path(ctx.h, path))
    try:
        T, st = api.icp_refine(xq, oq, xd, od, [0], [0], c["T0"][None], ctx=ctx, search=search, **prm)
    finally:
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
    return c, T[0], st[0]


def close_to(T, st, ref_T, ref):
    dR, dt, dr = np.abs(T[:, :3] - ref_T[:, :3]).max(), np.abs(T[:, 3] - ref_T[:, 3]).max(), abs(st["rmse"] - ref["rmse"])
    print("   max |dR| %.2e  max |dt| %.2e m  |d rmse| %.2e" % (dR, dt, dr))
    assert (st["status"], st["iters"], st["n_inl"]) == (ref["status"], ref["iters"], ref["n_inl"])
    assert st["fitness"] == ref["fitness"]
    assert dr <= TOL and dR <= TOL and dt <= TOL


@pytest.mark.parametrize("name", list(icp_cases.CASES))
def test_refinement_returns_the_split_paths_bytes(ctx, name):
    ref = icp_cases.reference(name)
    _, Tg, sg = refine(ctx, name, "grid")
    _, T2, s2 = refine(ctx, name, "brute", 2)
    assert Tg.tobytes() == T2.tobytes() and sg.tobytes() == s2.tobytes()
    _, Tg2, sg2 = refine(ctx, name, "grid", 2)                                        # the path does not reach the grid
    assert Tg2.tobytes() == Tg.tobytes() and sg2.tobytes() == sg.tobytes()
    for path in (0, 1):
        _, Tb, sb = refine(ctx, name, "brute", path)
        close_to(Tg, sg, Tb, sb)
    close_to(Tg, sg, ref["T"], ref)
    assert sg["status"] == _lib.ICP_CONVERGED


def test_refinement_status_paths(ctx):
    for over in (dict(max_iter=0), dict(max_corr=1e-4), dict(tol_rmse=0.0, tol_fitness=0.0, max_iter=12)):
        c, Tg, sg = refine(ctx, "box300_hand", "grid", **over)
        _, T2, s2 = refine(ctx, "box300_hand", "brute", 2, **over)
        assert Tg.tobytes() == T2.tobytes() and sg.tobytes() == s2.tobytes(), over
        want = {"max_iter": (_lib.ICP_MAX_ITER, over.get("max_iter")), "max_corr": (_lib.ICP_TOO_FEW, 0), "tol_rmse": (_lib.ICP_MAX_ITER, 12)}[next(iter(over))]
        assert (sg["status"], sg["iters"]) == want
        if "max_corr" in over or over.get("max_iter") == 0:
            assert np.array_equal(Tg, c["T0"])
    line = np.outer(np.arange(20.0), [1.0, 2.0, -1.0])
    xq, oq = icp_cases.csr([line + [0.01, 0, 0], np.zeros((0, 3))]); xd, od = icp_cases.csr([line])
    src, dst = [0, 1, -1, 0], [0, 0, 0, -1]
    T0 = np.stack([IDENT] * 4)
    res = {}
    for search in ("grid", "brute"):
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 2))
        try:
            res[search] = api.icp_refine(xq, oq, xd, od, src, dst, T0, max_iter=5, ctx=ctx, search=search)
        finally:
            ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
    T, st = res["grid"]
    assert T.tobytes() == res["brute"][0].tobytes() and st.tobytes() == res["brute"][1].tobytes()
    assert st["status"].tolist() == [_lib.ICP_DEGENERATE, _lib.ICP_TOO_FEW, _lib.ICP_NO_PAIR, _lib.ICP_NO_PAIR]
    assert st[0]["n_inl"] == 20 and st[0]["iters"] == 0 and np.array_equal(T, T0)
    T, st = api.icp_refine(xq, oq, xd, od, [], [], np.zeros((0, 3, 4)), ctx=ctx, search="grid")          # c = 0
    assert T.shape == (0, 3, 4) and len(st) == 0


# ------------------------------------------------------------------------------------------ 5. host and device forms, capture
def test_device_form_two_runs_and_graph_replay_give_identical_bits():
    names = ["box300_hand", "disk300_hand", "box2000_sc"]
    cs = [icp_cases.case(n) for n in names]
    xq, oq = icp_cases.csr([c["P"] for c in cs]); xd, od = icp_cases.csr([c["Q"] for c in cs])
    src = np.array([0, 1, 2, -1], np.int32); dst = np.array([0, 1, 2, 0], np.int32)
    T0 = np.stack([cs[max(s, 0)]["T0"] for s in src])
    T0b = T0.copy(); T0b[0] = rigid(0.5, (0.05, 0.0, -0.05)); T0b[1] = rigid(-0.5, (0.0, 0.0, 0.05))      # other seeds for the replay
    ms, md = max(len(c["P"]) for c in cs), max(len(c["Q"]) for c in cs)
    st_ = torch.cuda.Stream()
    with torch.cuda.stream(st_):
        cx = api.Context(0, stream=int(st_.cuda_stream))
        host_T, host_st = api.icp_refine(xq, oq, xd, od, src, dst, T0, ctx=cx, search="grid", **icp_cases.PARAMS)
        dT0 = dev(T0)
        args = (dev(xq), dev(oq, np.int64), dev(xd), dev(od, np.int64), dev(src, np.int32), dev(dst, np.int32), dT0, ms, md)
        kw = dict(ctx=cx, search="grid", **icp_cases.PARAMS)
        T1, s1 = api.icp_refine_torch(*args, **kw)                               # eager: also the covering warm-up
        T1, s1 = T1.clone(), s1.clone()
        T2, s2 = api.icp_refine_torch(*args, **kw)
        st_.synchronize()
        assert T1.cpu().numpy().tobytes() == T2.cpu().numpy().tobytes() and bytes(s1.cpu().numpy()) == bytes(s2.cpu().numpy())   # two runs
        assert T1.cpu().numpy().tobytes() == host_T.tobytes() and bytes(s1.cpu().numpy()) == host_st.tobytes()                # host == device
        assert cx.lib.pr_get_icp_search(cx.h) == _lib.ICP_SEARCH_BRUTE
        cx.check(cx.lib.pr_set_icp_search(cx.h, _lib.ICP_SEARCH_GRID))           # the mode of the capture is the context's
        kw["search"] = None
        out = (torch.zeros_like(T1), torch.zeros_like(s1))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st_):
            api.icp_refine_torch(*args, out=out, **kw)
        dT0.copy_(dev(T0b))                                                      # new T0 contents at the same addresses
        out[0].zero_(); out[1].zero_()
        g.replay()
        st_.synchronize()
        got = (out[0].cpu().numpy().copy(), bytes(out[1].cpu().numpy()))
        Te, se = api.icp_refine_torch(*args, **kw)                               # eager on the new seeds
        st_.synchronize()
        assert got[0].tobytes() == Te.cpu().numpy().tobytes() and got[1] == bytes(se.cpu().numpy())
        assert got[0].tobytes() != T1.cpu().numpy().tobytes()
        cx.close()


# ------------------------------------------------------------------------------------------ 6. verify_dev(search="grid")
def test_verify_dev_grid_equals_brute_on_the_generated_drive():
    import pose_drive
    from so_dso_place_recognition_amd.matcher import Matcher
    qs, ds, iq, idn, Rs, ts = pose_drive.drive()
    c = len(qs)
    xq, oq = icp_cases.csr(qs); xd, od = icp_cases.csr(ds)
    sig_q, sig_d = api.m2dp_generate(xq, iq, oq), api.m2dp_generate(xd, idn, od)
    fq, fd = api.cloud_frames(xq, iq, oq), api.cloud_frames(xd, idn, od)
    mt = Matcher("m2dp", c, c, ctx=api.Context(0, exact_statistics=True))
    mt.pack_database(dev(sig_d))
    idx, _ = mt.match(dev(sig_q), 0, 2.0, 2)
    res = {}
    for search in ("brute", "grid"):
        before = mt.ctx.lib.pr_get_icp_search(mt.ctx.h)
        out = mt.verify_dev(idx, (dev(xq), dev(oq, np.int64)), (dev(xd), dev(od, np.int64)), dev(fq), dev(fd), max(len(q) for q in qs),
                            max(len(d) for d in ds), hypotheses=2, max_corr=1.0, min_fitness=0.6, max_rmse=0.3, search=search)
        torch.cuda.synchronize()
        assert mt.ctx.lib.pr_get_icp_search(mt.ctx.h) == before == _lib.ICP_SEARCH_BRUTE
        res[search] = [o.cpu().numpy().copy() for o in out]
    (Tb, sb, ab, hb), (Tg, sg, ag, hg) = res["brute"], res["grid"]
    sb = np.frombuffer(sb.tobytes(), api.ICP_STATS); sg = np.frombuffer(sg.tobytes(), api.ICP_STATS)
    assert np.array_equal(ab, ag) and np.array_equal(hb, hg) and np.array_equal(sb["status"], sg["status"])
    assert np.array_equal(sb["iters"], sg["iters"]) and np.array_equal(sb["n_inl"], sg["n_inl"])
    print("   verify_dev grid against brute: max |dT| %.2e" % np.abs(Tb - Tg).max())
    assert np.abs(Tb - Tg).max() <= TOL
    assert ag[:, 0].all() and not ag[:, 1].any()
    mt.close()


# ------------------------------------------------------------------------------------------ 7. the executable
def test_cli_icp_search_grid_against_the_default(golden_dir, tmp_path):
    full = open(os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")).read().split("\n")
    poses = str(tmp_path / "poses_history_file.txt")
    open(poses, "w").write("\n".join(full[:60]) + "\n")
    pts = str(tmp_path / "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60)
    sig = str(tmp_path / "history_sc.txt")
    r = subprocess.run([os.path.join(BIN, "test_sc"), f"_poses_history_file:={poses}", f"_pts_history_file:={pts}", f"_sc_file:={sig}",
                        f"_incoming_id_file:={tmp_path / 'ids.txt'}", "_lidarRange:=45.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    base = [os.path.join(BIN, "match_signatures"), "--type", "sc", "--hist1", sig, "--hist2", sig, "--mask_width", "5", "--topk", "2",
            "--out", str(tmp_path / "out.txt"), "--poses1", poses, "--pts1", pts]
    got = {}
    for name, extra in (("default", []), ("grid", ["--icp_search", "grid"]), ("brute", ["--icp_search", "brute"])):
        icp = str(tmp_path / f"icp_{name}.txt")
        r = subprocess.run(base + ["--icp_out", icp] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got[name] = np.loadtxt(icp, ndmin=2)
    d, g = got["default"], got["grid"]
    assert d.shape == g.shape and d.shape[1] == 18 and (d[:, 2] != _lib.ICP_NO_PAIR).sum() > len(d) // 2
    assert np.array_equal(d[:, :5], g[:, :5])                                    # query, match, status, iters, fitness
    print("   --icp_search grid against the default: max |d rmse, dT| %.2e" % np.abs(d[:, 5:] - g[:, 5:]).max())
    assert np.abs(d[:, 5:] - g[:, 5:]).max() <= 1e-9
    assert np.array_equal(got["brute"], d)
    r = subprocess.run(base + ["--icp_out", str(tmp_path / "x.txt"), "--icp_search", "foo"], capture_output=True, text=True)
    assert r.returncode == 1 and "--icp_search" in r.stderr
