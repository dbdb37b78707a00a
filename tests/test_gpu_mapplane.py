"""The plane-metric map localiser on the device (pr_mapplane, mapplane.hip) against the restatement (mapplane_np.py): the
normals at the launch geometry's edges and over the committed cases, a refinement over every status and cloud size, the committed scene
beside the point form, one captured graph of fuse -> index -> normals -> seed -> refine replayed over a growing map, and keyframes of the
seq07 drive localised in the drive's own world map.  Guard words sit behind every output."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import icp_np
import maploc_np as mnp
import mapplane_np as pnp
import posegraph_np as pg
import worldmap_np as wnp
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_map import KCAP, MAXC, PCAP, dev, pose_inputs, same_bytes, seq07, stats_host  # noqa: F401  (seq07: the drive's fixture)
from test_gpu_maploc import EYE, GUARD, I32, World, assert_refine_matches, guarded, rigid
from test_mapplane_cpu import mp_angle

pytestmark = pytest.mark.gpu


class PlaneWorld(World):
    """test_gpu_maploc.py's world with a plane localiser over its localiser"""

    def __init__(self, ctx, ocap, cell, pair_capacity, max_src_pts):
        super().__init__(ctx, ocap, cell, pair_capacity, max_src_pts)
        self.pl = api.PlaneLocalizer(ctx, self.ml)

    def normals(self, ix, radius, min_nbrs, max_ratio, what, host_form=True):
        """device normals against the restatement: ninfo exactly, the normals byte for byte (and inside the angle bound against mpmath
        where a byte differs); two runs and the host form give the same bytes; -> (normals, ninfo) device tensors"""
        (nrm, g1), (info, g2) = guarded((self.ocap, 3), torch.float64), guarded((self.ocap,), torch.int32)
        self.pl.normals_torch(radius, min_nbrs, max_ratio, out=(nrm, info))
        torch.cuda.synchronize()
        g1(); g2()
        xyz, _, _ = self.host()
        wn, wi = pnp.normals(ix, xyz, radius, min_nbrs, max_ratio, self.ocap)
        gn, gi = nrm.cpu().numpy(), info.cpu().numpy()
        assert gi.tolist() == wi.tolist(), (what, np.flatnonzero(gi != wi)[:8], gi[gi != wi][:8], wi[gi != wi][:8])
        differ = np.flatnonzero((gn.view(np.int64) != wn.view(np.int64)).any(axis=1))
        for j in differ:                                  # a byte differs: the device's own bound against the mpmath eigenvector
            ang, bound = mp_angle(gn[j], pnp.row_neighbours(ix, xyz, int(j), radius)[0])
            print("   %s: row %d differs from the restatement by %.3g, %.3g from mpmath (bound %.3g)" % (what, j, np.abs(gn[j] - wn[j]).max(), ang, bound))
            assert wi[j] > 0 and ang <= bound, (what, j, ang, bound)
        assert len(differ) == 0, (what, "normals differ in bytes at rows", differ[:8])
        again = self.pl.normals_torch(radius, min_nbrs, max_ratio)
        torch.cuda.synchronize()
        assert same_bytes(again[0].cpu().numpy(), gn) and same_bytes(again[1].cpu().numpy(), gi), what
        if host_form:
            hn, hi = self.pl.normals(radius, min_nbrs, max_ratio)
            assert same_bytes(hn, gn) and same_bytes(hi, gi), what
        return nrm, info

    def close(self):
        self.pl.close()
        super().close()


# ------------------------------------------------------------------------------------------------ 1. the normals
@pytest.mark.parametrize("ocap,counts", [(32, (0, 1, 2, 3, 32)), (600, (255, 256, 257, 600))])
def test_normals_at_the_geometry_edges(ocap, counts):
    ctx = _stream_context(0)
    W = PlaneWorld(ctx, ocap, 1.0, 2, ocap)
    rng = np.random.default_rng(ocap)
    pts = pnp.plane_rows(rng, (0.5, 0.6, 0.62), 6.0 if ocap == 32 else 22.0, 40 * ocap, 1.0, noise=0.02, origin=(1.0, 0.5, 2.0))
    assert len(pts) >= ocap
    pts = pts[rng.permutation(len(pts))[:ocap]] if ocap == 600 else pts[:ocap]
    for R in counts:
        W.put(pts[:R])
        ix = W.index(("rows", R))
        _, info = W.normals(ix, 0.99, 4, 0.2, ("rows", R))
        info = info.cpu().numpy()
        assert (info[R:] == 0).all() and (info[:R] != 0).all()
        if R >= 32:
            assert (info > 0).any() and (info < 0).any()
    W.close(); ctx.close()


def test_normals_of_the_committed_cases():
    ctx = _stream_context(0)
    for name, (xyz, cell, radius, mn, mr) in pnp.normal_cases().items():
        ocap = 32 if len(xyz) <= 32 else 128
        W = PlaneWorld(ctx, ocap, cell, 2, 64)             # (the host form stages the world rows: out_capacity <= 2 x 64)
        W.put(xyz)
        ix = W.index(name)
        nrm, info = W.normals(ix, radius, mn, mr, name)
        if name == "the colliding keys":
            assert ix["info"].tolist() == [32, 32, 0, 0]
            for scribble, rows in ((1 << 30, 32), (-3, 0)):                                # state[0] is clamped before an address is formed
                W.put(xyz, state0=scribble)
                ix2 = W.index(("scribbled state", scribble))
                assert ix2["info"].tolist() == [rows, rows, 0, 0]
                _, i2 = W.normals(ix2, radius, mn, mr, ("scribbled state", scribble))
                assert (i2.cpu().numpy() != 0).sum() == rows
        if name == "plane unshifted":
            keep = nrm.cpu().numpy()
        if name == "plane shifted by 5e6":
            assert same_bytes(nrm.cpu().numpy(), keep)      # the offsets about the row itself are the same bits: so is the normal
        W.close()
    # radius (1 + 2^-10) > cell is refused before a launch, as are the other values, on a live handle
    W = PlaneWorld(ctx, 32, 1.0, 2, 16)
    lib, h = ctx.lib, W.pl.h
    b = (C.c_double * 64)()                             # host memory: every call below is refused before a launch
    err = lambda: lib.pr_last_error(ctx.h).decode()
    for r in (1.0, 0.9995):
        assert r * mnp.SLACK > 1.0
        assert lib.pr_mapplane_normals_dev(h, r, 5, 0.1, b, b) == _lib.PR_EINVAL and "exceeds the cell" in err(), r
    assert lib.pr_mapplane_normals_dev(h, 0.5, 2, 0.1, b, b) == _lib.PR_EINVAL and "min_nbrs=2" in err()
    assert lib.pr_mapplane_refine_dev(h, b, b, 1, b, 1, b, None, 5, 0.9995, 1e-6, 1e-6, 6, b, b, b, b) == _lib.PR_EINVAL and "exceeds the cell" in err()
    assert lib.pr_mapplane_refine_dev(h, b, b, 1, b, 3, b, None, 5, 0.5, 1e-6, 1e-6, 6, b, b, b, b) == _lib.PR_EINVAL and "c=3 outside" in err()
    assert lib.pr_mapplane_refine_dev(h, b, b, 1, b, 1, b, None, 5, 0.5, 1e-6, 1e-6, 5, b, b, b, b) == _lib.PR_EINVAL and "min_inliers=5 < 6" in err()
    assert lib.pr_mapplane_refine_dev(h, b, b, 1, b, 1, b, None, 5, 0.5, 1e-6, 1e-6, 6, None, b, b, b) == _lib.PR_EINVAL and "NULL" in err()
    other = _stream_context(0)
    with pytest.raises(ValueError, match="share one context"):
        api.PlaneLocalizer(other, W.ml)
    other.close()
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. a refinement
KW = dict(max_iter=30, max_corr=0.499, tol_rmse=1e-9, tol_fitness=1e-9, min_inliers=6)


def plane_refine(W, nrm, info, xq, oq, ps, T0, excl=None, in_place=False, **kw):
    c = len(ps)
    (T, i1), (st, i2) = guarded((c, 3, 4), torch.float64), guarded((c, api.ICP_STATS.itemsize), torch.uint8)
    if in_place:
        T.copy_(dev(T0).reshape(c, 3, 4))
    W.pl.refine_torch(dev(xq).reshape(-1, 3), dev(oq, np.int64), dev(ps, np.int32), T if in_place else dev(T0).reshape(c, 3, 4), nrm, info,
                      None if excl is None else dev(excl, np.int32).reshape(c, 2), out=(T, st), **kw)
    torch.cuda.synchronize()
    i1(); i2()
    return T.cpu().numpy(), stats_host(st)


@pytest.fixture(scope="module")
def refine_world():
    rc = pnp.refine_case()
    ctx = _stream_context(0)
    W = PlaneWorld(ctx, 1024, rc["cell"], 10, 513)
    W.put(rc["xyz"], rc["row"])
    ix = W.index("refine world")
    assert ix["info"].tolist() == [605, 605, 0, 0]
    nrm, info = W.normals(ix, what="refine world", **pnp.SCENE_NORMALS)
    assert info.cpu().numpy()[:605].tolist() == rc["ninfo"].tolist()
    wn, wi = pnp.normals(ix, W.host()[0], out_capacity=1024, **pnp.SCENE_NORMALS)
    yield rc, W, ix, nrm, info, pnp.table(wn, wi)
    W.close(); ctx.close()


def want_plane(rc, ix, normal_of, s, T0, excl=None, **kw):
    return pnp.icp_plane(ix, rc["xyz"], rc["row"], rc["xq"][rc["oq"][s]:rc["oq"][s + 1]], T0, normal_of, excl, **kw)


def test_refine_equals_the_restatement_over_sizes_statuses_and_pair_lists(refine_world):
    rc, W, ix, nrm, info, normal_of = refine_world
    xq, oq, Nq = rc["xq"], rc["oq"], 9
    CV, TF, DG, NP = _lib.ICP_CONVERGED, _lib.ICP_TOO_FEW, _lib.ICP_DEGENERATE, _lib.ICP_NO_PAIR
    status_of = [TF, TF, CV, CV, CV, CV, DG, TF, TF]          # sizes 0, 1, 255, 256, 257, 513 | one plane alone | no normals | 5 plane correspondents
    seed = lambda s: rc["seeds"][s] if 0 <= s < Nq else EYE
    calls = [[s] for s in range(Nq)] + [[5, 5, 3], [4, -1, 4, Nq, 2], [6, 7, 8, 0, 1, -1, Nq, 2, 3, 5]]
    cache = {}
    for ps in calls:
        T0 = np.stack([seed(s) for s in ps])
        T, st = plane_refine(W, nrm, info, xq, oq, ps, T0, **KW)
        for p, s in enumerate(ps):
            if not 0 <= s < Nq:
                assert st[p]["status"] == NP and same_bytes(T[p], EYE) and st[p]["n_inl"] == 0 and st[p]["fitness"] == 0.0
                continue
            if s not in cache:
                cache[s] = want_plane(rc, ix, normal_of, s, seed(s), **KW)
            assert st[p]["status"] == status_of[s], (ps, p, st[p]["status"])
            assert_refine_matches((T[p], st[p]), cache[s], (ps, p))
            if status_of[s] == CV:
                assert np.linalg.norm(T[p][:, 3] - rc["truth"][:, 3]) < 1e-9
            else:
                assert same_bytes(T[p], np.ascontiguousarray(seed(s)))                      # T is the last one a valid update produced
    assert cache[8]["n_plane"] == [5] and cache[7]["n_plane"] == [0] and cache[7]["n_inl"] == 40
    # in place, two runs, the host form: the same bytes
    ps = [5, 2, -1, 6, 8]
    T0 = np.stack([seed(s) for s in ps])
    T, st = plane_refine(W, nrm, info, xq, oq, ps, T0, **KW)
    T2, st2 = plane_refine(W, nrm, info, xq, oq, ps, T0, in_place=True, **KW)
    T3, st3 = plane_refine(W, nrm, info, xq, oq, ps, T0, **KW)
    hT, hst = W.pl.refine(xq, oq, ps, T0, nrm.cpu().numpy(), info.cpu().numpy(), **KW)
    for a, b in ((T2, st2), (T3, st3), (hT, hst)):
        assert a.tobytes() == T.tobytes() and b.tobytes() == st.tobytes()
    # MAX_ITER: two updates and no tolerance; an exclusion window per pair
    kw2 = dict(KW, max_iter=2, tol_rmse=0.0, tol_fitness=0.0)
    excl = [[1, 1], [3, 2], [0, 0]]
    T4, st4 = plane_refine(W, nrm, info, xq, oq, [5, 4, 4], np.stack([seed(5)] * 3), excl, **kw2)
    assert st4["status"].tolist() == [_lib.ICP_MAX_ITER] * 3 and st4["iters"].tolist() == [2, 2, 2]
    for p, s in enumerate([5, 4, 4]):
        assert_refine_matches((T4[p], st4[p]), want_plane(rc, ix, normal_of, s, seed(5), tuple(excl[p]), **kw2), ("excl", p))
    assert T4[1].tobytes() != T4[2].tobytes()
    T5, st5 = plane_refine(W, nrm, info, xq, oq, [5], seed(5)[None], [[1, 1]], **KW)
    assert_refine_matches((T5[0], st5[0]), want_plane(rc, ix, normal_of, 5, seed(5), (1, 1), **KW), "window, converged")
    assert st5[0]["status"] == CV
    assert W.pl.refine_torch(dev(xq), dev(oq, np.int64), dev([], np.int32), dev(np.zeros((0, 3, 4))), nrm, info, **KW)[0].shape == (0, 3, 4)


def test_the_pass_is_the_localisers_search(refine_world):
    """max_iter = 0 is the final pass alone: its n_inl and rmse are formed from the (j, d2) of the pass, which must be pr_maploc_nn_dev's
    bytes - the count, and the tree sum of every d2, with and without an exclusion window"""
    rc, W, ix, nrm, info, normal_of = refine_world
    xq, oq = rc["xq"], rc["oq"]
    for excl in (None, [[1, 2]]):
        for s in (4, 5):
            T0 = rc["seeds"][s][None]
            T, st = plane_refine(W, nrm, info, xq, oq, [s], T0, excl, **dict(KW, max_iter=0))
            _, j, d2 = W.nn(xq, oq, [s], T0, excl, mc=KW["max_corr"])
            terms = np.zeros((len(j), pnp.SUMS))
            terms[:, 0], terms[:, 1] = j >= 0, np.where(j >= 0, d2, 0.0)
            sums = pnp.tree_sum(terms)
            assert st[0]["status"] == _lib.ICP_MAX_ITER and st[0]["iters"] == 0 and same_bytes(T[0], np.ascontiguousarray(T0[0]))
            assert st[0]["n_inl"] == int(sums[0]) == (j >= 0).sum() and st[0]["fitness"] == sums[0] / len(j)
            assert abs(st[0]["rmse"] - math.sqrt(sums[1] / sums[0])) <= 1e-15, (s, excl, st[0]["rmse"], math.sqrt(sums[1] / sums[0]))


def test_the_scene_point_to_plane_halves_the_point_forms_translation_error():
    sc = pnp.corner_scene()
    ctx = _stream_context(0)
    W = PlaneWorld(ctx, 512, sc["cell"], 2, 1024)
    W.put(sc["xyz"], sc["row"])
    ix = W.index("scene")
    nrm, info = W.normals(ix, what="scene", **pnp.SCENE_NORMALS)
    xq, oq = sc["src"], np.array([0, len(sc["src"])], np.int64)
    T, st = plane_refine(W, nrm, info, xq, oq, [0], sc["seed"][None], **KW)
    pT, pst = W.ml.refine_torch(dev(xq), dev(oq, np.int64), dev([0], np.int32), dev(sc["seed"][None]), **dict(KW, min_inliers=3))
    torch.cuda.synchronize()
    pT, pst = pT.cpu().numpy(), stats_host(pst)
    ep, eq = (float(np.linalg.norm(t[0][:, 3] - sc["truth"][:, 3])) for t in (T, pT))
    print("   translation error: point-to-plane %.3g m (%d iterations), point-to-point %.3g m (%d iterations)" % (ep, st[0]["iters"], eq, pst[0]["iters"]))
    assert st[0]["status"] == pst[0]["status"] == _lib.ICP_CONVERGED and ep <= 0.5 * eq
    assert_refine_matches((T[0], st[0]), pnp.icp_plane(ix, sc["xyz"], sc["row"], sc["src"], sc["seed"], pnp.table(*pnp.normals(ix, sc["xyz"], **pnp.SCENE_NORMALS)), **KW), "scene")
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. one captured graph
def test_one_graph_of_fuse_index_normals_seed_refine_over_a_growing_map():
    rng = np.random.default_rng(61)
    pts = []
    for plane in (2, 0, 1):                                                                # a floor and two walls, 3 m each way
        pts.append(np.insert(3.0 * rng.random((500, 2)), plane, 0.05, axis=1))
    shape = np.vstack(pts)
    clouds = []
    for k in range(3):
        P = rigid(rng, 0.3, 1.0)
        clouds.append(((shape[rng.permutation(len(shape))[:290]] @ P[:, :3].T + P[:, 3]), rng.random(290).astype(np.float32), P.reshape(12)))
    pert = np.stack([rigid(rng, 0.005, 0.03) for _ in range(3)])
    kw = dict(max_iter=12, max_corr=0.4, tol_rmse=1e-7, tol_fitness=1e-7, min_inliers=6)
    nkw = dict(radius=0.499, min_nbrs=4, max_ratio=0.05)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, 4, 1024, 300)
        wm = api.WorldMap(ctx, km, 1024)
        ml = api.MapLocalizer(ctx, wm, 0.5, 3, 300)
        pl = api.PlaneLocalizer(ctx, ml)
        idx, rel = dev([0, 1, 2], np.int32), dev(pert)
        (finfo, g1), (iinfo, g2) = guarded((4,), torch.int64), guarded((4,), torch.int64)
        (nrm, g7), (ninfo, g8) = guarded((1024, 3), torch.float64), guarded((1024,), torch.int32)
        (T0, g3), (ps, g4) = guarded((3, 3, 4), torch.float64), guarded((3,), torch.int32)
        (T, g5), (stats, g6) = guarded((3, 3, 4), torch.float64), guarded((3, api.ICP_STATS.itemsize), torch.uint8)
        outs = (finfo, iinfo, nrm, ninfo, T0, ps, T, stats)

        def chain():
            wm.fuse_torch(cell=0.5, min_count=1, keep="first", info=finfo)
            ml.index_torch(info=iinfo)
            pl.normals_torch(out=(nrm, ninfo), **nkw)
            ml.seed_torch(km.poses, km.state, idx, T_rel=rel, out=(T0, ps))
            pl.refine_torch(km.xyz, km.offs, ps, T0, nrm, ninfo, out=(T, stats), **kw)

        def snapshot():
            st.synchronize()
            for g in (g1, g2, g3, g4, g5, g6, g7, g8):
                g()
            return [t.cpu().numpy().copy() for t in outs]

        chain()                                                                            # eager once (the empty map), then the capture - on the empty map
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            chain()
        for count in range(4):
            if count:
                x, it, pose = clouds[count - 1]
                km.append(x, it, np.array([0, len(x)], np.int64), np.zeros((1, 16)), poses=pose.reshape(1, 12), ids=[count])
            for t in outs:
                t.fill_(GUARD)
            g.replay()
            replayed = snapshot()
            for t in outs:
                t.fill_(GUARD)
            chain()
            eager = snapshot()
            for a, b in zip(replayed, eager):
                assert a.tobytes() == b.tobytes(), count
            mx, mi, mo, mp_ = km.xyz.cpu().numpy(), km.inten.cpu().numpy(), km.offs.cpu().numpy(), km.poses.cpu().numpy()
            world = wnp.fuse(mx, mi, mo, mp_, count, 0.5, 1, "first", out_capacity=1024)
            R = int(world["info"][0])
            wx = wm.xyz.cpu().numpy()                                                      # the rows the device fused (its bytes, the restatement's to rounding)
            ix = mnp.index(wx, R, 0.5, 1024)
            assert replayed[1].tolist() == ix["info"].tolist() and ix["info"][2] == 0
            wn, wi = pnp.normals(ix, wx, out_capacity=1024, **nkw)
            assert replayed[3].tolist() == wi.tolist() and replayed[2].tobytes() == wn.tobytes(), count
            wT0, wps = mnp.seed(mp_, count, [0, 1, 2], None, pert, None)
            assert replayed[4].tobytes() == wT0.tobytes() and replayed[5].tolist() == wps.tolist() == [p if p < count else -1 for p in range(3)]
            got = stats_host(torch.from_numpy(replayed[7]))
            for p in range(3):
                if p < count:
                    want = pnp.icp_plane(ix, wx, wm.row.cpu().numpy(), mx[mo[p]:mo[p + 1]], wT0[p], pnp.table(wn, wi), **kw)
                    assert_refine_matches((replayed[6][p], got[p]), want, (count, p))
                    assert got[p]["fitness"] > 0.5 and got[p]["status"] in (_lib.ICP_CONVERGED, _lib.ICP_MAX_ITER)
                else:
                    assert got[p]["status"] == _lib.ICP_NO_PAIR and replayed[6][p].tobytes() == EYE.tobytes()
        del g
        pl.close(); ml.close(); wm.close(); km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the drive
DRIVE_ROWS = (40, 109)


def test_keyframes_of_the_drive_localised_with_the_plane_metric(seq07):
    """The seq07 drive of test_gpu_maploc.py; keyframes 40 and 109 from seeds turned by 1 degree and shifted by 0.3 m through
    PlaneLocalizer.localize_torch, beside the point form on the same inputs (reported, no threshold).  The drive's cloud is a sparse
    visual-odometry one: fused at cell 1.0 - test_gpu_maploc.py's world - a few dozen rows of 7723 have four neighbours within the cell,
    so the plane form has almost nothing to work with there; fused at cell 3.0 about a third of the rows get a normal."""
    ctx = _stream_context(0)
    win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
    km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
    out = win.empty_out()
    for p in range(len(seq07["pid"])):
        w, x, it, k, pid = pose_inputs(seq07, p)
        win.push_torch(dev(w), dev(x), dev(it, np.float32), I32(k), out=out)
        km.append_push(out, pose=dev(w), id=I32(pid))
    OC = 1 << 16
    mo = km.offs.cpu().numpy()
    ms = int(np.diff(mo[:111]).max())
    for CELL, min_valid in ((1.0, 0), (3.0, 100)):
        wm = api.WorldMap(ctx, km, OC)
        winfo = wm.fuse_torch(cell=CELL, min_count=1, keep="first")
        ml = api.MapLocalizer(ctx, wm, CELL, 4, ms)
        pl = api.PlaneLocalizer(ctx, ml)
        ml.index_torch()
        nkw = dict(radius=0.99 * CELL, min_nbrs=4, max_ratio=0.3)
        nrm, ninfo = pl.normals_torch(**nkw)
        torch.cuda.synchronize()
        R = int(winfo.cpu()[0])
        xyz, row = wm.xyz.cpu().numpy()[:R], wm.row.cpu().numpy()[:R]
        ix = mnp.index(xyz, R, CELL)
        lazy = pnp.LazyNormals(ix, xyz, **nkw)
        gi, gn = ninfo.cpu().numpy(), nrm.cpu().numpy()
        for j in np.random.default_rng(1).integers(0, R, 300):                                 # a sample of the device's normals against the restatement
            wi, wn = lazy(j)
            assert gi[j] == wi and gn[j].tobytes() == np.array(wn).tobytes(), j
        assert (gi[:R] > 0).sum() >= min_valid and (gi[R:] == 0).all()
        mx, mp_ = km.xyz.cpu().numpy(), km.poses.cpu().numpy()
        c = len(DRIVE_ROWS)
        pert = np.zeros((c, 3, 4))
        for p, a in enumerate(np.array([(0, 1, 0), (1, 1, 1)], np.float64)):
            a = a / np.linalg.norm(a)
            pert[p, :, :3] = pg.exp_so3(a * np.deg2rad(1.0)); pert[p, :, 3] = 0.3 * a[[1, 2, 0]]
        idx = dev(DRIVE_ROWS, np.int32)
        kw = dict(max_iter=30, max_corr=0.9, tol_rmse=1e-6, tol_fitness=1e-6)
        wT0, wps = mnp.seed(mp_, 110, DRIVE_ROWS, None, pert, DRIVE_ROWS)
        truth = np.stack([pg.inv(mp_[r].reshape(3, 4)) for r in DRIVE_ROWS])
        T, stats, acc = pl.localize_torch(km.xyz, km.offs, km.poses, km.state, idx, nrm, ninfo, T_rel=dev(pert), src=idx, min_inliers=6,
                                          min_fitness=0.6, max_rmse=0.5, **kw)
        pT, pstats, _ = ml.localize_torch(km.xyz, km.offs, km.poses, km.state, idx, T_rel=dev(pert), src=idx, min_inliers=3, min_fitness=0.6,
                                          max_rmse=0.5, **kw)
        torch.cuda.synchronize()
        T0, ps = (t.cpu().numpy() for t in pl.last_localize["seed"])
        assert T0.tobytes() == wT0.tobytes() and ps.tolist() == list(DRIVE_ROWS)
        T, stats, acc, pT, pstats = T.cpu().numpy(), stats_host(stats), acc.cpu().numpy(), pT.cpu().numpy(), stats_host(pstats)
        for p, r in enumerate(DRIVE_ROWS):
            want = pnp.icp_plane(ix, xyz, row, mx[mo[r]:mo[r + 1]], wT0[p], lazy, min_inliers=6, **kw)
            print("   cell %g (%d rows, %d with a normal), row %3d: %d points, largest entry of T - inv(P_r): seed %.3g, point-to-plane %.3g (fitness %.3f rmse %.3g iters %d status %d), "
                  "point-to-point %.3g (iters %d status %d); plane correspondents in the first pass %d"
                  % (CELL, R, (gi[:R] > 0).sum(), r, mo[r + 1] - mo[r], np.abs(wT0[p] - truth[p]).max(), np.abs(T[p] - truth[p]).max(), stats[p]["fitness"], stats[p]["rmse"],
                     stats[p]["iters"], stats[p]["status"], np.abs(pT[p] - truth[p]).max(), pstats[p]["iters"], pstats[p]["status"], want["n_plane"][0]))
            assert_refine_matches((T[p], stats[p]), want, r)
            assert bool(acc[p]) == mnp.accept(want, 0.6, 0.5), r
        pl.close(); ml.close(); wm.close()
    km.close(); win.close(); ctx.close()
