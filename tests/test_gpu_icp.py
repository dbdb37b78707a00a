"""The ICP refinement on the device (csrc/icp.hip: pr_icp_nn*, pr_icp_pairs* and their Python forms) against the restatement icp_np.py.
Correspondences: indices and d2 EQUAL bit for bit under every launch geometry (pr_set_icp_path).  Refinement on the committed cases
(icp_cases.py): status, iters, n_inl and fitness equal; rmse, R and t within 1e-10 absolute (metres for t) - 100 x the 1e-12 that the order
of the restatement's own sums may move them (test_icp_cpu.py), and four orders below the 2.4e-6 m by which one wrong 1 cm correspondence
among 4096 points moves t."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import icp_cases
import icp_np
from resident_fuzz_cases import bits_equal
from so_dso_place_recognition_amd import _lib, api

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "so_dso_place_recognition_amd", "bin")
PATHS = (0, 1, 2)          # pr_set_icp_path: by shape | every workgroup scans the whole target | split target + combine
TOL = 1e-10
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def bits(a, b):
    return bits_equal(a, b)


def rigid(deg, t, axis=(0.3, -0.8, 0.5)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.hstack([np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K, np.asarray(t, np.float64)[:, None]])


def nn_all_paths(ctx, clouds_q, clouds_d, pairs, T):
    """icp_nn under the three geometries, each equal to the restatement bit for bit; returns the restatement's (offs, idx, d2)."""
    xq, oq = icp_cases.csr(clouds_q)
    xd, od = icp_cases.csr(clouds_d)
    ps = np.array([p[0] for p in pairs], np.int32); pd = np.array([p[1] for p in pairs], np.int32)
    offs, wi, wd = [0], [], []
    for (s, d), Ti in zip(pairs, T):
        if s < 0 or d < 0:
            offs.append(offs[-1]); continue
        j, v = icp_np.nn(icp_np.transform(Ti, clouds_q[s]), clouds_d[d])
        wi.append(j); wd.append(v); offs.append(offs[-1] + len(j))
    wi = np.concatenate(wi) if wi else np.zeros(0, np.int32); wd = np.concatenate(wd) if wd else np.zeros(0)
    for path in PATHS:
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, path))
        try:
            go, gi, gd = api.icp_nn(xq, oq, xd, od, ps, pd, np.asarray(T), ctx=ctx)
        finally:
            ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
        assert np.array_equal(go, offs), (path, go, offs)
        assert np.array_equal(gi, wi), (path, np.flatnonzero(gi != wi)[:8])
        assert bits(gd, wd), path
    return np.array(offs), wi, wd


# ------------------------------------------------------------------------------------------ 4. correspondences, bit for bit
def test_icp_nn_sizes_shared_sources_and_missing_pairs(ctx):
    tile = api.icp_tile_rows()
    assert tile >= 64
    rng = np.random.default_rng(1)
    src_sizes = (0, 1, 2, 3, 63, 64, 65, 257)
    dst_sizes = (0, 1, tile - 1, tile, tile + 1, 2 * tile + 3)
    cq = [rng.normal(0, 5, (n, 3)) for n in src_sizes]
    cd = [rng.normal(0, 5, (n, 3)) for n in dst_sizes]
    pairs = [(s, d) for s in range(len(cq)) for d in range(len(cd))]                  # every source cloud in several pairs
    pairs += [(-1, 2), (3, -1), (-1, -1), (7, 5)]
    T = [IDENT if i % 3 == 0 else rigid(7.0 * (i % 5) + 1, rng.normal(0, 1, 3)) for i in range(len(pairs))]
    offs, wi, wd = nn_all_paths(ctx, cq, cd, pairs, T)
    assert offs[-1] == sum(src_sizes) * len(dst_sizes) + 257
    empty_target = [i for i, (s, d) in enumerate(pairs) if d == 0 and s >= 0]
    for i in empty_target:
        assert np.all(wi[offs[i]:offs[i + 1]] == -1) and np.all(np.isinf(wd[offs[i]:offs[i + 1]]))


def test_icp_nn_exact_ties_go_to_the_first_index(ctx):
    tile = api.icp_tile_rows()
    rng = np.random.default_rng(2)
    grid = rng.integers(-2, 3, (2 * tile + 40, 3)).astype(np.float64)               # many exact copies, across tiles and splits
    src = rng.integers(-2, 3, (300, 3)).astype(np.float64)
    offs, wi, wd = nn_all_paths(ctx, [src], [grid], [(0, 0)], [IDENT])
    first = {tuple(g): j for j, g in reversed(list(enumerate(grid)))}
    hit = [i for i, p in enumerate(src) if tuple(p) in first]
    assert len(hit) > 100 and all(wi[i] == first[tuple(src[i])] and wd[i] == 0.0 for i in hit)
    assert np.array_equal(wd, np.round(wd))


def test_icp_nn_nan_and_inf_coordinates_never_win(ctx):
    tile = api.icp_tile_rows()
    rng = np.random.default_rng(3)
    src = rng.normal(0, 3, (130, 3)); dst = rng.normal(0, 3, (tile + 70, 3))
    src[5, 1] = np.nan; src[6, 0] = np.inf; src[7] = -np.inf
    dst[0, 2] = np.nan; dst[3, 0] = np.inf; dst[tile, 1] = -np.inf; dst[tile + 1] = np.nan
    all_bad = np.full((9, 3), np.nan); all_bad[::2] = np.inf
    offs, wi, wd = nn_all_paths(ctx, [src, src[:20]], [dst, all_bad], [(0, 0), (1, 1), (0, 1)], [rigid(11, (0.5, -0.2, 0.1)), IDENT, IDENT])
    assert wi[5] == -1 and wi[6] == -1 and wi[7] == -1 and np.isinf(wd[5])
    assert not np.isin(wi[:130], (0, 3, tile, tile + 1)).any()
    assert np.all(wi[130:] == -1) and np.all(np.isinf(wd[130:]))


# ------------------------------------------------------------------------------------------ 5. refinement against the restatement
def refine_case(ctx, name, path=0, **over):
    c = icp_cases.case(name)
    xq, oq = icp_cases.csr([c["P"]]); xd, od = icp_cases.csr([c["Q"]])
    prm = dict(icp_cases.PARAMS); prm.update(over)
    ctx.check(ctx.lib.pr_set_icp_path(ctx.h, path))
    try:
        T, st = api.icp_refine(xq, oq, xd, od, [0], [0], c["T0"][None], ctx=ctx, **prm)
    finally:
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
    return c, T[0], st[0]


def close_to(T, st, ref):
    dR, dt, dr = np.abs(T[:, :3] - ref["T"][:, :3]).max(), np.abs(T[:, 3] - ref["T"][:, 3]).max(), abs(st["rmse"] - ref["rmse"])
    print("   max |dR| %.2e  max |dt| %.2e m  |d rmse| %.2e" % (dR, dt, dr))
    assert (st["status"], st["iters"], st["n_inl"]) == (ref["status"], ref["iters"], ref["n_inl"])
    assert st["fitness"] == ref["fitness"]
    assert dr <= TOL and dR <= TOL and dt <= TOL


@pytest.mark.parametrize("name", list(icp_cases.CASES))
def test_icp_refine_equals_the_restatement(ctx, name):
    ref = icp_cases.reference(name)
    for path in PATHS:
        c, T, st = refine_case(ctx, name, path)
        close_to(T, st, ref)
    e0, e1 = icp_cases.pose_error(c["T0"], c["R"], c["t"]), icp_cases.pose_error(T, c["R"], c["t"])
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)


def test_icp_refine_batch_of_all_cases_with_a_missing_pair(ctx):
    names = list(icp_cases.CASES)
    cs = [icp_cases.case(n) for n in names]
    xq, oq = icp_cases.csr([c["P"] for c in cs]); xd, od = icp_cases.csr([c["Q"] for c in cs])
    src = np.array([0, 1, -1, 2, 3, 4, 5], np.int32); dst = np.array([0, 1, 3, 2, 3, 4, 5], np.int32)
    T0 = np.stack([cs[max(s, 0)]["T0"] for s in src])
    T, st = api.icp_refine(xq, oq, xd, od, src, dst, T0, ctx=ctx, **icp_cases.PARAMS)
    for i, s in enumerate(src):
        if s < 0:
            assert st[i]["status"] == _lib.ICP_NO_PAIR and np.array_equal(T[i], T0[i]) and st[i]["n_inl"] == 0 and st[i]["iters"] == 0
        else:
            close_to(T[i], st[i], icp_cases.reference(names[s]))


def test_many_pairs_take_the_four_points_per_lane_kernel(ctx):
    """More than 4096 workgroups at one point per lane: the kernel with four points per lane (chunks of 1024 points) runs.  Correspondences
    bit-equal as ever; the refinement of 4100 copies of a committed case agrees with the restatement and is the same in every pair."""
    c = 4100
    case = icp_cases.case("box300_hand")
    ref = icp_cases.reference("box300_hand")
    xq, oq = icp_cases.csr([case["P"]]); xd, od = icp_cases.csr([case["Q"]])
    src = np.zeros(c, np.int32); dst = np.zeros(c, np.int32)
    Tn = rigid(2.0, (0.2, 0.0, -0.1))
    j, v = icp_np.nn(icp_np.transform(Tn, case["P"]), case["Q"])
    for path in PATHS:
        ctx.check(ctx.lib.pr_set_icp_path(ctx.h, path))
        try:
            go, gi, gd = api.icp_nn(xq, oq, xd, od, src, dst, np.tile(Tn, (c, 1, 1)), ctx=ctx)
        finally:
            ctx.check(ctx.lib.pr_set_icp_path(ctx.h, 0))
        assert np.array_equal(go, np.arange(c + 1) * len(j))
        assert np.array_equal(gi.reshape(c, -1), np.tile(j, (c, 1))) and bits(gd.reshape(c, -1), np.tile(v, (c, 1))), path
    T, st = api.icp_refine(xq, oq, xd, od, src, dst, np.tile(case["T0"], (c, 1, 1)), ctx=ctx, **icp_cases.PARAMS)
    close_to(T[0], st[0], ref)
    assert bits(T, np.tile(T[0], (c, 1, 1))) and st.tobytes() == st[:1].tobytes() * c


# ------------------------------------------------------------------------------------------ 6. status paths
def test_status_paths(ctx):
    ref0 = icp_np.icp(icp_cases.case("box300_hand")["P"], icp_cases.case("box300_hand")["Q"], IDENT, max_iter=0, max_corr=1.0)
    c, T, st = refine_case(ctx, "box300_hand", max_iter=0)
    assert np.array_equal(T, c["T0"]) and st["status"] == _lib.ICP_MAX_ITER and st["iters"] == 0
    assert st["n_inl"] == ref0["n_inl"] and st["fitness"] == ref0["fitness"] and abs(st["rmse"] - ref0["rmse"]) <= TOL
    c, T, st = refine_case(ctx, "box300_hand", max_corr=1e-4)
    assert st["status"] == _lib.ICP_TOO_FEW and st["iters"] == 0 and np.array_equal(T, c["T0"]) and st["n_inl"] < 3
    c, T, st = refine_case(ctx, "box300_hand", tol_rmse=0.0, tol_fitness=0.0, max_iter=12)
    ref = icp_np.icp(c["P"], c["Q"], c["T0"], max_iter=12, max_corr=1.0, tol_rmse=0.0, tol_fitness=0.0)
    assert st["status"] == _lib.ICP_MAX_ITER and st["iters"] == 12
    close_to(T, st, ref)
    line = np.outer(np.arange(20.0), [1.0, 2.0, -1.0])
    xq, oq = icp_cases.csr([line + [0.01, 0, 0], np.zeros((0, 3))]); xd, od = icp_cases.csr([line])
    T, st = api.icp_refine(xq, oq, xd, od, [0, 1], [0, 0], np.stack([IDENT, IDENT]), max_iter=5, ctx=ctx)
    assert st[0]["status"] == _lib.ICP_DEGENERATE and st[0]["iters"] == 0 and np.array_equal(T[0], IDENT) and st[0]["n_inl"] == 20
    assert st[1]["status"] == _lib.ICP_TOO_FEW and st[1]["fitness"] == 0.0 and st[1]["rmse"] == 0.0 and st[1]["n_inl"] == 0
    T, st = api.icp_refine(xq, oq, xd, od, [], [], np.zeros((0, 3, 4)), ctx=ctx)          # c = 0
    assert T.shape == (0, 3, 4) and len(st) == 0


# ------------------------------------------------------------------------------------------ 7. other forms
def stats_host(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), api.ICP_STATS)


def test_device_form_graph_replay_and_two_runs_give_identical_bits():
    names = ["box300_hand", "disk300_hand", "box2000_sc"]
    cs = [icp_cases.case(n) for n in names]
    xq, oq = icp_cases.csr([c["P"] for c in cs]); xd, od = icp_cases.csr([c["Q"] for c in cs])
    src = np.array([0, 1, 2, -1], np.int32); dst = np.array([0, 1, 2, 0], np.int32)
    T0 = np.stack([cs[max(s, 0)]["T0"] for s in src])
    ms, md = max(len(c["P"]) for c in cs), max(len(c["Q"]) for c in cs)
    st_ = torch.cuda.Stream()
    with torch.cuda.stream(st_):
        cx = api.Context(0, stream=int(st_.cuda_stream))
        host_T, host_st = api.icp_refine(xq, oq, xd, od, src, dst, T0, ctx=cx, **icp_cases.PARAMS)
        args = (dev(xq), dev(oq, np.int64), dev(xd), dev(od, np.int64), dev(src, np.int32), dev(dst, np.int32), dev(T0), ms, md)
        kw = dict(ctx=cx, **icp_cases.PARAMS)
        T1, s1 = api.icp_refine_torch(*args, **kw)                               # eager: also the covering warm-up
        T1, s1 = T1.clone(), s1.clone()
        T2, s2 = api.icp_refine_torch(*args, **kw)
        st_.synchronize()
        assert bits(T1.cpu().numpy(), T2.cpu().numpy()) and bytes(s1.cpu().numpy()) == bytes(s2.cpu().numpy())       # two runs
        assert bits(T1.cpu().numpy(), host_T) and bytes(s1.cpu().numpy()) == host_st.tobytes()                      # host form == device form
        out = (torch.zeros_like(T1), torch.zeros_like(s1))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st_):
            api.icp_refine_torch(*args, out=out, **kw)
        out[0].zero_(); out[1].zero_()
        g.replay()
        st_.synchronize()
        assert bits(out[0].cpu().numpy(), T1.cpu().numpy()) and bytes(out[1].cpu().numpy()) == bytes(s1.cpu().numpy())
        assert stats_host(s1)["status"].tolist() == [0, 0, 0, _lib.ICP_NO_PAIR]
        for i, n in enumerate(names):
            close_to(T1[i].cpu().numpy(), stats_host(s1)[i], icp_cases.reference(n))
        cx.close()


# ------------------------------------------------------------------------------------------ 8. end to end
def drive(c=6, P=3000, seed=201):
    """c places seen twice: the DB clouds and the queries (moved by a planted rigid motion, jittered, 90 % subsets).  Every physical point
    keeps its intensity in both views (a constant intensity would leave SC's intensity channel - bin mean > cloud average - all zero, and
    the fused score NaN)."""
    from test_align import _scene, _yaw
    rng = np.random.default_rng(seed)
    qs, ds, iqs, ids, Rs, ts = [], [], [], [], [], []
    for i in range(c):
        base = _scene(rng, P)
        inten = rng.random(P).astype(np.float32)
        R, t = _yaw(rng.random() * 2 * np.pi), np.array([rng.normal(0, 3), rng.normal(0, 0.2), rng.normal(0, 3)])
        keep = rng.random(P) < 0.9
        q = base[keep]
        qs.append(q + rng.normal(0, 0.02, q.shape)); iqs.append(inten[keep])
        keep = rng.random(P) < 0.9
        d = base[keep]
        ds.append(d @ R.T + t + rng.normal(0, 0.02, d.shape)); ids.append(inten[keep])
        Rs.append(R); ts.append(t)
    return qs, ds, np.concatenate(iqs), np.concatenate(ids), Rs, ts


def test_matcher_match_align_verify_on_a_generated_drive():
    from so_dso_place_recognition_amd.matcher import Matcher
    qs, ds, iq, idn, Rs, ts = drive()
    c = len(qs)
    xq, oq = icp_cases.csr(qs); xd, od = icp_cases.csr(ds)
    sig_q, sig_d = api.sc_generate(xq, iq, oq), api.sc_generate(xd, idn, od)
    fq, fd = api.cloud_frames(xq, iq, oq), api.cloud_frames(xd, idn, od)
    mt = Matcher("sc", c, c, ctx=api.Context(0, exact_statistics=True))
    mt.pack_database(dev(sig_d))
    idx, _ = mt.match(dev(sig_q), 0, 2.0, 2)
    T, stats, acc = mt.verify(idx, (dev(xq), dev(oq, np.int64)), (dev(xd), dev(od, np.int64)), fq, fd, max(len(q) for q in qs),
                              max(len(d) for d in ds), max_corr=1.0, min_fitness=0.6, max_rmse=0.3)
    torch.cuda.synchronize()
    ix = idx.cpu().numpy(); T = T.cpu().numpy(); acc = acc.cpu().numpy(); st = stats_host(stats).reshape(c, 2)
    assert np.array_equal(ix[:, 0], np.arange(c))
    var, _ = mt.align(idx)
    hT, hst, hacc = api.verify_matches((xq, oq), (xd, od), ix, var.cpu().numpy()[..., 0], fq, fd, 1.0, 0.6, 0.3, ctx=mt.ctx)
    assert bits(T, hT) and st.tobytes() == hst.tobytes() and np.array_equal(acc, hacc)       # the same chain through api.verify_matches
    for i in range(c):
        er, et = icp_cases.pose_error(T[i, 0], Rs[i], ts[i])
        print("  place", i, "status", st[i, 0]["status"], "iters", st[i, 0]["iters"], "fitness %.3f rmse %.3f" % (st[i, 0]["fitness"], st[i, 0]["rmse"]),
              "err %.3f deg %.3f m" % (er, et), "| second candidate accepted:", bool(acc[i, 1]))
        assert acc[i, 0] and er < 0.2 and et < 0.05
        assert not acc[i, 1]                                                    # another place does not verify
    mt.close()


def test_cli_icp_out_equals_verify_matches(golden_dir, tmp_path):
    full = open(os.path.join(golden_dir, "kitti_seq07", "poses_history_file.txt")).read().split("\n")
    poses = str(tmp_path / "poses_history_file.txt")
    open(poses, "w").write("\n".join(full[:60]) + "\n")
    pts = str(tmp_path / "pts_history_file.txt")
    helpers.write_synthetic_points(poses, pts, per_pose=60)
    sig = str(tmp_path / "history_sc.txt")
    r = subprocess.run([os.path.join(BIN, "test_sc"), f"_poses_history_file:={poses}", f"_pts_history_file:={pts}", f"_sc_file:={sig}",
                        f"_incoming_id_file:={tmp_path / 'ids.txt'}", "_lidarRange:=45.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out, icp = str(tmp_path / "out.txt"), str(tmp_path / "icp.txt")
    k = 2
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", "sc", "--hist1", sig, "--hist2", sig, "--mask_width", "5", "--topk", str(k),
                        "--out", out, "--icp_out", icp, "--poses1", poses, "--pts1", pts], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    h = np.loadtxt(sig)
    m = len(h)
    ix = np.loadtxt(out).reshape(m, k, 2)[..., 0].astype(np.int32)
    xyz, it, offs, _ = api.pts_preprocess(poses, pts, None, 45.0, False, gpu=True)
    assert len(offs) - 1 == m
    var, _ = api.match_align("sc", h, h, ix)
    fr = api.cloud_frames(xyz, it, offs)
    T, st, _ = api.verify_matches((xyz, offs), (xyz, offs), ix, var[..., 0], fr, fr)
    got = np.loadtxt(icp, ndmin=2)
    assert got.shape == (m * k, 18)
    want = np.concatenate([np.repeat(np.arange(m), k)[:, None], np.where(st["status"].reshape(-1, 1) == _lib.ICP_NO_PAIR, -1, ix.reshape(-1, 1)),
                           st["status"].reshape(-1, 1), st["iters"].reshape(-1, 1), st["fitness"].reshape(-1, 1), st["rmse"].reshape(-1, 1),
                           T.reshape(m * k, 12)], 1).astype(np.float64)
    assert bits(got, want), np.abs(got - want).max(0)
    assert (st["status"] != _lib.ICP_NO_PAIR).sum() > m                         # most pairs were refined
    r = subprocess.run([os.path.join(BIN, "match_signatures"), "--type", "m2dp", "--hist1", sig, "--hist2", sig, "--out", out, "--icp_out", icp,
                        "--poses1", poses, "--pts1", pts], capture_output=True, text=True)
    assert r.returncode == 1 and "--icp_out" in r.stderr
