"""The map localiser on the device (pr_maploc, maploc.hip) against the NumPy restatement (maploc_np.py) and against the
existing ICP calls on the same one-cloud target: the index at the launch geometry's edges, under hash collisions and at the rule's edges;
a correspondence pass bit for bit (and equal to pr_icp_nn_radius in both search modes where nothing is excluded or duplicated); a
refinement byte-equal to pr_icp_pairs under search="grid"; the seed rule; one captured graph of fuse -> index -> seed -> refine replayed
over a growing map; and keyframes of the seq07 drive localised in the drive's own world map.  Guard words sit behind every output."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_np
import maploc_np as mnp
import posegraph_np as pg
import worldmap_np as wnp
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_map import KCAP, MAXC, PCAP, dev, pose_inputs, same_bytes, seq07, stats_host  # noqa: F401  (seq07: the drive's fixture)

pytestmark = pytest.mark.gpu

GUARD = -7
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])
LIM = float(1 << 20)
I32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")


def guarded(shape, dtype, extra=8):
    """(view of `shape`, check()): the view lies in front of `extra` guard words"""
    n = int(np.prod(shape))
    big = torch.full((n + extra,), GUARD, dtype=dtype, device="cuda")

    def intact():
        assert bool((big[n:] == GUARD).all()), ("guard words behind an output", shape, dtype)
    return big[:n].view(*shape), intact


class World:
    """a world map whose rows the test writes itself, and a localiser over it"""

    def __init__(self, ctx, ocap, cell, pair_capacity, max_src_pts):
        self.ctx, self.ocap, self.cell, self.ms = ctx, ocap, cell, max_src_pts
        self.km = api.KeyframeMap(ctx, 4, 64, 16)
        self.wm = api.WorldMap(ctx, self.km, ocap)
        self.ml = api.MapLocalizer(ctx, self.wm, cell, pair_capacity, max_src_pts)

    def put(self, xyz, row=None, state0=None):
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        R = len(xyz)
        self.wm.xyz.fill_(float("nan"))                  # a row behind the count that were read would show as SKIPPED
        self.wm.row.fill_(GUARD)
        if R:
            self.wm.xyz[:R] = dev(xyz)
            self.wm.row[:R] = dev(np.zeros(R) if row is None else row, np.int32)
        self.wm.state[0] = R if state0 is None else state0

    def host(self):
        torch.cuda.synchronize()
        return self.wm.xyz.cpu().numpy(), self.wm.row.cpu().numpy(), int(self.wm.state.cpu().numpy()[0])

    def index(self, what):
        """one device index against the restatement; the host form and count() agree; -> the restatement's index"""
        info, intact = guarded((4,), torch.int64)
        self.ml.index_torch(info=info)
        xyz, row, s0 = self.host()
        ix = mnp.index(xyz, s0, self.cell, self.ocap)
        assert info.cpu().numpy().tolist() == ix["info"].tolist(), (what, info.cpu().numpy(), ix["info"])
        intact()
        assert self.ml.count() == (int(ix["info"][0]), int(ix["info"][2])), what
        assert self.ml.index().tolist() == ix["info"].tolist(), what
        return ix

    def nn(self, xq, oq, ps, T, excl=None, mc=0.5):
        c, rows = len(ps), len(ps) * max(self.ms, 1)
        (oo, i1), (ji, i2), (dd, i3) = guarded((c + 1,), torch.int64), guarded((rows,), torch.int32), guarded((rows,), torch.float64)
        self.ml.nn_torch(dev(xq).reshape(-1, 3), dev(oq, np.int64), dev(ps, np.int32), dev(T).reshape(c, 3, 4),
                         None if excl is None else dev(excl, np.int32).reshape(c, 2), mc, out=(oo, ji, dd))
        torch.cuda.synchronize()
        i1(); i2(); i3()
        oo, ji, dd = oo.cpu().numpy(), ji.cpu().numpy(), dd.cpu().numpy()
        total = int(oo[-1])
        assert (ji[total:] == GUARD).all() and (dd[total:] == GUARD).all(), "rows behind the call's"
        return oo, ji[:total], dd[:total]

    def want_nn(self, ix, xq, oq, ps, T, excl=None, mc=0.5):
        xyz, row, _ = self.host()
        xq = np.asarray(xq, np.float64).reshape(-1, 3)
        offs, js, ds = [0], [], []
        for p, s in enumerate(ps):
            if 0 <= s < len(oq) - 1:
                P = xq[oq[s]:oq[s + 1]][:self.ms]
                j, d = mnp.nn(ix, xyz, row, icp_np.transform(T[p], P), mc, None if excl is None else tuple(excl[p]))
                js.append(j); ds.append(d)
                offs.append(offs[-1] + len(P))
            else:
                offs.append(offs[-1])
        return (np.array(offs, np.int64), np.concatenate(js + [np.zeros(0, np.int32)]).astype(np.int32), np.concatenate(ds + [np.zeros(0)]))

    def existing_nn(self, xq, oq, ps, T, excl=None, mc=0.5, search="grid"):
        """pr_icp_nn_radius on (the world rows the windows leave, [0, rows], one cloud), pair by pair, indices mapped back"""
        xyz, row, s0 = self.host()
        R = min(max(s0, 0), self.ocap)
        Nq = len(oq) - 1
        offs, js, ds = [0], [], []
        for p, s in enumerate(ps):
            keep = np.arange(R) if excl is None else np.nonzero(~((excl[p][0] <= row[:R]) & (row[:R] <= excl[p][1])))[0]
            o, j, d = api.icp_nn_radius(xq, oq, xyz[keep], [0, len(keep)], [s if 0 <= s < Nq else -1], [0], np.asarray(T[p]).reshape(1, 3, 4), mc,
                                        ctx=self.ctx, search=search)
            js.append(np.where(j >= 0, keep[np.maximum(j, 0)] if len(keep) else -1, -1)); ds.append(d)
            offs.append(offs[-1] + int(o[1]))
        return (np.array(offs, np.int64), np.concatenate(js + [np.zeros(0, np.int32)]).astype(np.int32), np.concatenate(ds + [np.zeros(0)]))

    def close(self):
        self.ml.close(); self.wm.close(); self.km.close()


def assert_nn_equal(got, want, what):
    assert got[0].tolist() == want[0].tolist(), (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, np.flatnonzero(got[1] != want[1])[:8])
    assert got[2].tobytes() == want[2].tobytes(), what


def one_per_voxel(seed, rows, spread, cell=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    seen, pts = set(), []
    while len(pts) < rows:
        p = rng.normal(0, spread, 3) + offset
        k = tuple(np.floor(p / cell).astype(int))
        if k not in seen:
            seen.add(k); pts.append(p)
    return np.array(pts).reshape(-1, 3)


def rigid(rng, rot, shift):
    T = np.zeros((3, 4))
    T[:, :3] = pg.exp_so3(rng.normal(0, rot, 3)); T[:, 3] = rng.normal(0, shift, 3)
    return T


def self_pass(W, ix, what):
    """every world row as a source point under the identity: an indexed row finds itself (or the smaller row of its voxel) at d2 = 0"""
    xyz, row, s0 = W.host()
    R = min(max(s0, 0), W.ocap)
    args = (xyz[:max(R, 1)], [0, R], [0], EYE[None])               # (an empty world: one unused row, so that the set has an address)
    got, want = W.nn(*args), W.want_nn(ix, *args)
    assert_nn_equal(got, want, what)
    return got


# ------------------------------------------------------------------------------------------------ 1. the index
@pytest.mark.parametrize("ocap,counts", [(32, (0, 1, 2, 32)), (600, (255, 256, 257, 600))])
def test_index_at_the_geometry_edges(ocap, counts):
    assert 1 << mnp.log2T(ocap) == (64 if ocap == 32 else 2048)
    ctx = _stream_context(0)
    W = World(ctx, ocap, 1.0, 2, ocap)
    pts = one_per_voxel(ocap, ocap, 3.0 if ocap == 32 else 6.0)
    for R in counts:
        W.put(pts[:R], np.arange(R) // 7)
        ix = W.index(("rows", R))
        assert ix["info"].tolist() == [R, R, 0, 0]
        got = self_pass(W, ix, ("self", R))
        assert got[1].tolist() == list(range(R)) and (got[2] == 0).all()
    W.close(); ctx.close()


def test_index_colliding_keys_rule_edges_and_a_coarser_cell():
    ctx = _stream_context(0)
    W = World(ctx, 32, 1.0, 2, 32)
    cells = np.array(mnp.COLLIDING_CELLS, np.float64)    # ten keys with the home slot 62 of the T = 64 table: the chain wraps its end
    W.put(cells + 0.5)
    ix = W.index("colliding keys")
    assert ix["info"].tolist() == [32, 32, 0, 0] and set(ix["first"]) == set(mnp.COLLIDING_CELLS)
    assert self_pass(W, ix, "colliding keys")[1].tolist() == list(range(32))
    edge = np.zeros((14, 3)) + 0.5
    edge[0] = (np.nan, 1, 1); edge[1] = (2, np.inf, 2); edge[2] = (3, 3, -np.inf)
    edge[3] = (LIM, 0.5, 0.5); edge[4] = (LIM - 1, 0.5, 0.5); edge[5] = (-LIM, 0.5, 0.5); edge[6] = (0.5, np.nextafter(LIM, 0), 0.5); edge[7] = (0.5, 0.5, -LIM - 1)
    edge[8] = (-0.0, -0.0, -0.0); edge[9] = (0.0, 0.25, 0.0); edge[10] = (-1e-300, 0.5, 0.5); edge[11] = (3.5, 3.5, 3.5); edge[12] = (-3.5, -3.5, -3.5)
    edge[13] = (0.5, 0.5, 0.5)
    W.put(edge)
    ix = W.index("rule edges")
    assert ix["info"].tolist() == [7, 14, mnp.SKIPPED | mnp.RANGE | mnp.DUPLICATE, 0]       # rows 8, 9, 13 share the voxel (0, 0, 0)
    assert sorted(ix["first"].values()) == [4, 5, 6, 8, 10, 11, 12]                         # 2^20 - 1 and -2^20 kept, 2^20 and -2^20 - 1 not
    got = self_pass(W, ix, "rule edges")
    assert got[1].tolist() == [-1, -1, -1, -1, 4, 5, 6, -1, 8, 8, 10, 11, 12, -1]           # (row 13 is 0.866 from row 8, the row of its voxel)
    for scribble, rows in ((1 << 30, 32), (-3, 0)):                                        # state[0] is clamped before an address is formed
        W.put(cells + 0.5, state0=scribble)
        ix = W.index(("scribbled state", scribble))
        assert ix["info"].tolist() == [rows, rows, 0, 0]
    W.close()
    # rows as a fuse at cell 0.5 leaves them, indexed at cell 1.0: DUPLICATE, the candidates are the smallest j per key
    W = World(ctx, 600, 1.0, 2, 600)
    fine = one_per_voxel(9, 500, 2.0, cell=0.5)
    W.put(fine, np.arange(500) % 5)
    ix = W.index("coarser cell")
    assert ix["info"][2] == mnp.DUPLICATE and 50 < ix["info"][0] < 450 and ix["info"][1] == 500
    got = self_pass(W, ix, "coarser cell")
    assert (got[1][ix["rows"]] == ix["rows"]).all() and (got[2][ix["rows"]] == 0).all()     # an indexed row finds itself; the others are no candidates
    assert not np.isin(got[1][got[1] >= 0], np.setdiff1d(np.arange(500), ix["rows"])).any()
    rng = np.random.default_rng(10)
    src = fine[rng.integers(0, 500, 300)] + rng.normal(0, 0.3, (300, 3))
    args = (src, [0, 300], [0, 0], np.stack([EYE, rigid(rng, 0.02, 0.1)]), [[1, 2], [3, 0]], 0.9)
    assert_nn_equal(W.nn(*args), W.want_nn(ix, *args), "coarser cell, a window")
    W.put(one_per_voxel(9, 500, 6.0))
    assert W.index("clean again")["info"].tolist() == [500, 500, 0, 0]                     # the flag is the call's: nothing is sticky
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. one pass
SIZES = (0, 1, 255, 256, 257, 513)


def pass_world():
    """540 scattered rows around the origin and, far from them, the rows the edge cases aim at; keyframe rows 0 .. 5"""
    base = one_per_voxel(21, 540, 4.0)
    special = np.array([(50.25, 50.25, 50.25),                                   # 540: the target at exactly max_corr, and one ulp inside
                        (60.75, 60.5, 60.5), (61.25, 60.5, 60.5),               # 541, 542: two rows at equal distance
                        (69.75, 69.75, 69.75), (70.25, 70.25, 70.25),           # 543, 544: around a voxel corner
                        (LIM - 0.125, 0.5, 0.5), (-LIM, 0.5, 0.5)])             # 545, 546: the first and the last voxel of the range
    xyz = np.vstack([base, special])
    return xyz, (np.arange(len(xyz)) * 6 // len(xyz)).astype(np.int32)


def pass_sources(xyz):
    rng = np.random.default_rng(22)
    clouds = [xyz[rng.integers(0, 540, s)] + rng.normal(0, 0.2, (s, 3)) for s in SIZES]
    e = clouds[5]
    e[0] = (50.75, 50.25, 50.25); e[1] = (np.nextafter(50.75, 0), 50.25, 50.25); e[2] = (49.75, 50.25, 50.25)
    e[3] = (61.0, 60.5, 60.5); e[4] = (70.0, 70.0, 70.0); e[5] = (70.0, 70.3, 70.3); e[6] = (70.0, 70.0, 70.3)
    e[7] = (np.nan, 0, 0); e[8] = (0, np.inf, 0); e[9] = (1e300, 0, 0); e[10] = (-1e300, 1e300, 0)
    e[11] = (LIM + 0.25, 0.5, 0.5); e[12] = (-LIM - 0.25, 0.5, 0.5); e[13] = (LIM + 1.25, 0.5, 0.5); e[14] = (-LIM - 1.25, 0.5, 0.5)
    e[15] = (LIM - 0.5, 0.5, 0.5)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    return np.vstack(clouds), offs


def test_pass_equals_the_restatement_and_the_existing_search():
    ctx = _stream_context(0)
    xyz, row = pass_world()
    W = World(ctx, 600, 1.0, 6, 513)                    # (the host form stages the whole query set: pair_capacity >= Nq)
    W.put(xyz, row)
    ix = W.index("pass world")
    assert ix["info"].tolist() == [547, 547, 0, 0]
    xq, oq = pass_sources(xyz)
    Nq = len(SIZES)
    rng = np.random.default_rng(23)
    # the edge cloud under the identity: exact distance, tie, corner, NaN / Inf / 1e300 sources, the voxels around the range's ends
    args = (xq, oq, [5], EYE[None])
    got = W.nn(*args)
    assert_nn_equal(got, W.want_nn(ix, *args), "edges")
    assert got[1][:16].tolist() == [-1, 540, -1, 541, 543, 544, 544, -1, -1, -1, -1, 545, 546, -1, -1, 545]
    assert got[2][1] < 0.25 and got[2][3] == 0.0625 and np.isinf(got[2][0])
    for mode in ("brute", "grid"):
        assert_nn_equal(got, W.existing_nn(*args, search=mode), ("edges", mode))
    # every cloud size, c = 1, 3, 5 with shared sources, pairs that are off, a NaN entry in T
    Ts = np.stack([rigid(rng, 0.02, 0.1) for _ in range(5)])
    nanT = Ts.copy(); nanT[1, 2, 1] = np.nan
    calls = [([s], Ts[:1]) for s in range(Nq)] + [([5, 5, 3], Ts[:3]), ([4, -1, 4, Nq, 2], Ts), ([0, 1, 5, 5, 5], Ts), ([3, 3, 3], nanT[:3]),
                                                   ([-1], Ts[:1]), ([Nq + 7, -5], Ts[:2])]
    for ps, T in calls:
        args = (xq, oq, ps, T)
        got = W.nn(*args)
        assert_nn_equal(got, W.want_nn(ix, *args), ps)
        for mode in ("brute", "grid"):
            assert_nn_equal(got, W.existing_nn(*args, search=mode), (ps, mode))
    assert W.nn(xq, oq, [], np.zeros((0, 3, 4)))[0].tolist() == [0]
    # exclusion windows: the nearest row's keyframe, every row, nothing (lo > hi), one per pair
    near = int(row[W.nn(xq, oq, [4], EYE[None])[1].max()])
    for ps, excl in (([4], [[near, near]]), ([4], [[0, 5]]), ([4], [[3, 2]]), ([5, 4, 3], [[0, 0], [5, 5], [1, 4]]), ([2, -1, 5], [[2, 2], [0, 5], [-9, 99]])):
        T = np.stack([EYE] * len(ps))
        args = (xq, oq, ps, T, excl)
        got = W.nn(*args)
        assert_nn_equal(got, W.want_nn(ix, *args), (ps, excl))
        assert_nn_equal(got, W.existing_nn(*args, search="grid"), (ps, excl, "existing"))
    assert (W.nn(xq, oq, [4], EYE[None], [[0, 5]])[1] == -1).all() and (W.nn(xq, oq, [4], EYE[None], [[3, 2]])[1] >= 0).any()
    # a cloud longer than max_src_pts is read up to it
    W2 = World(ctx, 600, 1.0, 2, 300)
    W2.put(xyz, row); ix2 = W2.index("short")
    args = (xq, oq, [5, 3], Ts[:2])
    got = W2.nn(*args)
    assert got[0].tolist() == [0, 300, 556]
    assert_nn_equal(got, W2.want_nn(ix2, *args), "max_src_pts")
    # the host form
    ho, hj, hd = W.ml.nn(xq, oq, [5, -1, 3], Ts[:3], excl=[[0, 0], [0, 0], [2, 1]], max_corr=0.5)
    assert_nn_equal((ho, hj, hd), W.want_nn(ix, xq, oq, [5, -1, 3], Ts[:3], [[0, 0], [0, 0], [2, 1]]), "host form")
    W2.close(); W.close(); ctx.close()


def test_live_handle_refusals():
    ctx, other = _stream_context(0), _stream_context(0)
    W = World(other, 64, 1.0, 2, 16)
    with pytest.raises(ValueError, match="share one context"):
        api.MapLocalizer(ctx, W.wm, 1.0, 2, 16)
    lib, h = other.lib, W.ml.h
    b = (C.c_double * 64)()
    err = lambda: lib.pr_last_error(other.h).decode()
    assert lib.pr_maploc_nn_dev(h, b, b, 1, b, 3, b, None, 0.5, b, b, b) == _lib.PR_EINVAL and "c=3 outside 0 .. pair_capacity=2" in err()
    assert lib.pr_maploc_nn_dev(h, b, b, 1, b, -1, b, None, 0.5, b, b, b) == _lib.PR_EINVAL and "c=-1 outside" in err()
    assert lib.pr_maploc_seed_dev(h, b, b, 4, b, None, None, None, 3, b, b) == _lib.PR_EINVAL and "c=3 outside" in err()
    assert lib.pr_maploc_refine_dev(h, b, b, 1, b, 3, b, None, 5, 0.5, 1e-6, 1e-6, 3, b, b) == _lib.PR_EINVAL and "c=3 outside" in err()
    # max_corr (1 + 2^-10) > cell, on values whose product is above 1 in fp64 beyond doubt: b is host memory, so every call here must be
    # one that is refused before a launch
    for mc in (1.0, 0.9995):
        assert mc * mnp.SLACK > 1.0
        assert lib.pr_maploc_nn_dev(h, b, b, 1, b, 1, b, None, mc, b, b, b) == _lib.PR_EINVAL and "exceeds the cell" in err(), mc
        assert lib.pr_maploc_refine_dev(h, b, b, 1, b, 1, b, None, 5, mc, 1e-6, 1e-6, 3, b, b) == _lib.PR_EINVAL and "exceeds the cell" in err()
    assert lib.pr_maploc_nn_dev(h, b, None, 1, b, 1, b, None, 0.5, b, b, b) == _lib.PR_EINVAL and "NULL" in err()
    assert lib.pr_maploc_nn_dev(h, b, b, 1, b, 1, b, None, 0.5, None, b, b) == _lib.PR_EINVAL and "NULL" in err()
    assert lib.pr_maploc_index_dev(h, None) == _lib.PR_EINVAL and "d_info is NULL" in err()
    assert lib.pr_maploc_seed_dev(h, None, b, 4, b, None, None, None, 1, b, b) == _lib.PR_EINVAL and "NULL" in err()
    with pytest.raises(ValueError, match="exceeds pair_capacity"):
        W.ml.nn_torch(dev(np.zeros((4, 3))), dev([0, 4], np.int64), dev([0, 0, 0], np.int32), dev(np.zeros((3, 3, 4))))
    W.close(); other.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. a refinement
def refine_case():
    """a world of 700 scattered rows (one per voxel of cell 1.0) and, far away, six rows on a line; sources: two clouds cut from the
    world and moved, a cloud far from everything, a cloud along the line"""
    rng = np.random.default_rng(31)
    base = one_per_voxel(31, 700, 4.0)
    line = np.array([(100.5 + i, 100.5, 100.5) for i in range(6)])
    xyz = np.vstack([base, line])
    row = (np.arange(len(xyz)) * 4 // len(xyz)).astype(np.int32)
    clouds = []
    for s, (rot, shift) in ((300, (0.02, 0.1)), (257, (0.03, 0.15))):
        M = rigid(rng, rot, shift)                                                         # the cloud is the world seen through inv(M)
        q = base[rng.permutation(700)[:s]] + rng.normal(0, 0.01, (s, 3))
        clouds.append((q - M[:, 3]) @ M[:, :3])
    clouds.append(rng.normal(0, 1.0, (40, 3)) + 500.0)
    clouds.append(line + (0.1, 0.0, 0.0))
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return xyz, row, np.vstack(clouds), offs


def dev_refine(W, xq, oq, ps, T0, excl=None, in_place=False, **kw):
    c = len(ps)
    (T, i1), (st, i2) = guarded((c, 3, 4), torch.float64), guarded((c, api.ICP_STATS.itemsize), torch.uint8)
    if in_place:
        T.copy_(dev(T0).reshape(c, 3, 4))
    W.ml.refine_torch(dev(xq).reshape(-1, 3), dev(oq, np.int64), dev(ps, np.int32), T if in_place else dev(T0).reshape(c, 3, 4),
                      None if excl is None else dev(excl, np.int32).reshape(c, 2), out=(T, st), **kw)
    torch.cuda.synchronize()
    i1(); i2()
    return T.cpu().numpy(), stats_host(st)


def assert_refine_matches(got, want, what):
    """device (T, stats record) against a restatement's result: the decisions equal, the sums within 1e-10"""
    T, s = got
    for k in ("status", "iters", "n_inl"):
        assert int(s[k]) == want[k], (what, k, int(s[k]), want[k])
    assert float(s["fitness"]) == want["fitness"], (what, "fitness")
    assert abs(float(s["rmse"]) - want["rmse"]) <= 1e-10, (what, "rmse", float(s["rmse"]), want["rmse"])
    assert np.abs(T - want["T"]).max() <= 1e-10, (what, "T", np.abs(T - want["T"]).max())


def test_refine_equals_the_existing_grid_search_and_the_restatement():
    ctx = _stream_context(0)
    xyz, row, xq, oq = refine_case()
    W = World(ctx, 1024, 1.0, 6, 300)
    W.put(xyz, row)
    ix = W.index("refine world")
    assert ix["info"].tolist() == [706, 706, 0, 0]
    ps = [0, 1, -1, 2, 3, 4]                                                               # two that converge, NO_PAIR, TOO_FEW, DEGENERATE, NO_PAIR (= Nq)
    T0 = np.stack([EYE] * 6)
    kw = dict(max_iter=30, max_corr=0.9, tol_rmse=1e-6, tol_fitness=1e-6, min_inliers=3)
    T, st = dev_refine(W, xq, oq, ps, T0, **kw)
    assert st["status"].tolist() == [_lib.ICP_CONVERGED, _lib.ICP_CONVERGED, _lib.ICP_NO_PAIR, _lib.ICP_TOO_FEW, _lib.ICP_DEGENERATE, _lib.ICP_NO_PAIR]
    assert st["fitness"][0] > 0.9 and st["fitness"][1] > 0.9 and same_bytes(T[2], EYE) and st[2]["n_inl"] == 0 and st[2]["fitness"] == 0.0
    # the existing call on the same one-cloud target, search = grid: equal bytes
    eT, est = api.icp_refine(xq, oq, xyz, [0, len(xyz)], [0, 1, -1, 2, 3, -1], [0] * 6, T0, ctx=ctx, search="grid", **kw)
    assert T.tobytes() == eT.tobytes() and st.tobytes() == est.tobytes()
    for p, s in enumerate(ps):
        if 0 <= s < 4:
            assert_refine_matches((T[p], st[p]), mnp.icp(ix, xyz, row, xq[oq[s]:oq[s + 1]], T0[p], **kw), ("pair", p))
    # in place, two runs, the host form
    T2, st2 = dev_refine(W, xq, oq, ps, T0, in_place=True, **kw)
    T3, st3 = dev_refine(W, xq, oq, ps, T0, **kw)
    hT, hst = W.ml.refine(xq, oq, ps, T0, **kw)
    for a, b in ((T2, st2), (T3, st3), (hT, hst)):
        assert a.tobytes() == T.tobytes() and b.tobytes() == st.tobytes()
    # MAX_ITER: two updates and no tolerance; an exclusion window against the restatement and the existing call on the filtered rows
    kw2 = dict(kw, max_iter=2, tol_rmse=0.0, tol_fitness=0.0)
    excl = [[1, 1], [3, 2], [0, 0]]
    T4, st4 = dev_refine(W, xq, oq, [0, 1, 1], T0[:3], excl, **kw2)
    assert st4["status"].tolist() == [_lib.ICP_MAX_ITER] * 3 and st4["iters"].tolist() == [2, 2, 2]
    for p, s in enumerate([0, 1, 1]):
        assert_refine_matches((T4[p], st4[p]), mnp.icp(ix, xyz, row, xq[oq[s]:oq[s + 1]], T0[p], tuple(excl[p]), **kw2), ("excl", p))
        keep = np.nonzero(~((excl[p][0] <= row) & (row <= excl[p][1])))[0]
        eT, est = api.icp_refine(xq, oq, xyz[keep], [0, len(keep)], [s], [0], T0[p:p + 1], ctx=ctx, search="grid", **kw2)
        assert T4[p].tobytes() == eT[0].tobytes() and st4[p].tobytes() == est[0].tobytes(), p
    assert T4[1].tobytes() != T4[2].tobytes()
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the seed
def test_seed_equals_the_restatement():
    ctx = _stream_context(0)
    W = World(ctx, 64, 1.0, 8, 16)
    rng = np.random.default_rng(41)
    kcap = 6
    poses = np.stack([rigid(rng, 1.0, 30.0) for _ in range(kcap)]).reshape(kcap, 12)
    poses[4, 6] = np.nan
    T_rel = np.stack([rigid(rng, 0.3, 2.0) for _ in range(8)])
    T_rel[6, 0, 3] = np.nan
    idx = np.array([0, 3, -1, 5, 4, 2, 1, 6], np.int32)
    acc = np.array([1, 1, 1, 0, 1, 1, 1, 1], np.uint8)
    src = np.array([7, 6, 5, 4, 3, 2, 1, 0], np.int32)
    for n in (6, 5, 99, 0, -2):                          # idx 5 is the count at n = 5; 99 is clamped to the capacity
        for a, t, s in ((acc, T_rel, src), (None, T_rel, None), (acc, None, src), (None, None, None)):
            (T0, i1), (ps, i2) = guarded((8, 3, 4), torch.float64), guarded((8,), torch.int32)
            W.ml.seed_torch(dev(poses), I32(n), dev(idx, np.int32), None if a is None else dev(a, np.uint8).bool(), None if t is None else dev(t),
                            None if s is None else dev(s, np.int32), out=(T0, ps))
            torch.cuda.synchronize()
            i1(); i2()
            wT, wp = mnp.seed(poses, n, idx, a, t, s)
            assert ps.cpu().numpy().tolist() == wp.tolist(), (n, ps, wp)
            assert T0.cpu().numpy().tobytes() == wT.tobytes(), n
    assert mnp.seed(poses, 6, idx, acc, T_rel, src)[1].tolist() == [7, 6, -1, -1, -1, 2, -1, -1]
    W.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. one captured graph
def test_one_graph_of_fuse_index_seed_refine_over_a_growing_map():
    rng = np.random.default_rng(51)
    shape = one_per_voxel(51, 400, 2.5, cell=0.5)                                          # one scene, seen from three poses
    clouds = []
    for k in range(3):
        P = rigid(rng, 0.3, 1.0)
        clouds.append(((shape[rng.permutation(400)[:250]] @ P[:, :3].T + P[:, 3]), rng.random(250).astype(np.float32), P.reshape(12)))
    pert = np.stack([rigid(rng, 0.01, 0.05) for _ in range(3)])
    kw = dict(max_iter=12, max_corr=0.4, tol_rmse=1e-6, tol_fitness=1e-6, min_inliers=3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, 4, 1024, 300)
        wm = api.WorldMap(ctx, km, 1024)
        ml = api.MapLocalizer(ctx, wm, 0.5, 3, 300)
        idx, rel = dev([0, 1, 2], np.int32), dev(pert)
        (finfo, g1), (iinfo, g2) = guarded((4,), torch.int64), guarded((4,), torch.int64)
        (T0, g3), (ps, g4) = guarded((3, 3, 4), torch.float64), guarded((3,), torch.int32)
        (T, g5), (stats, g6) = guarded((3, 3, 4), torch.float64), guarded((3, api.ICP_STATS.itemsize), torch.uint8)

        def chain():
            wm.fuse_torch(cell=0.5, min_count=1, keep="first", info=finfo)
            ml.index_torch(info=iinfo)
            ml.seed_torch(km.poses, km.state, idx, T_rel=rel, out=(T0, ps))
            ml.refine_torch(km.xyz, km.offs, ps, T0, out=(T, stats), **kw)

        def snapshot():
            st.synchronize()
            for g in (g1, g2, g3, g4, g5, g6):
                g()
            return [t.cpu().numpy().copy() for t in (finfo, iinfo, T0, ps, T, stats)]

        chain()                                                                            # eager once (the empty map), then the capture - on the empty map
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            chain()
        for count in range(4):
            if count:
                x, it, pose = clouds[count - 1]
                km.append(x, it, np.array([0, len(x)], np.int64), np.zeros((1, 16)), poses=pose.reshape(1, 12), ids=[count])
            for t in (finfo, iinfo, T0, ps, T, stats):
                t.fill_(GUARD)
            g.replay()
            replayed = snapshot()
            for t in (finfo, iinfo, T0, ps, T, stats):
                t.fill_(GUARD)
            chain()
            eager = snapshot()
            for a, b in zip(replayed, eager):
                assert a.tobytes() == b.tobytes(), count
            mx, mi, mo, mp = km.xyz.cpu().numpy(), km.inten.cpu().numpy(), km.offs.cpu().numpy(), km.poses.cpu().numpy()
            world = wnp.fuse(mx, mi, mo, mp, count, 0.5, 1, "first", out_capacity=1024)
            assert replayed[0].tolist() == world["info"].tolist()
            R = int(world["info"][0])
            ix = mnp.index(world["xyz"], R, 0.5)
            assert replayed[1].tolist() == ix["info"].tolist() and ix["info"][2] == 0
            wT0, wps = mnp.seed(mp, count, [0, 1, 2], None, pert, None)
            assert replayed[2].tobytes() == wT0.tobytes() and replayed[3].tolist() == wps.tolist() == [p if p < count else -1 for p in range(3)]
            got = stats_host(torch.from_numpy(replayed[5]))
            for p in range(3):
                if p < count:
                    want = mnp.icp(ix, world["xyz"], world["row"], mx[mo[p]:mo[p + 1]], wT0[p], **kw)
                    assert_refine_matches((replayed[4][p], got[p]), want, (count, p))
                    assert got[p]["fitness"] > 0.5
                else:
                    assert got[p]["status"] == _lib.ICP_NO_PAIR and replayed[4][p].tobytes() == EYE.tobytes()
        del g
        ml.close(); wm.close(); km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the drive
DRIVE_ROWS = (1, 40, 80, 109)


def test_keyframes_of_the_drive_localised_in_its_world_map(seq07):
    """The seq07 drive of test_gpu_map.py (110 keyframes) fused under the map's poses at cell 1.0, min_count 1, keep first; keyframes 1, 40,
    80 and 109 localised from seeds turned by 1 degree and shifted by 0.3 m, without exclusion and with the keyframe's own rows excluded."""
    ctx = _stream_context(0)
    win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
    km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
    out = win.empty_out()
    for p in range(len(seq07["pid"])):
        w, x, it, k, pid = pose_inputs(seq07, p)
        win.push_torch(dev(w), dev(x), dev(it, np.float32), I32(k), out=out)
        km.append_push(out, pose=dev(w), id=I32(pid))
    keys, points, flags = km.count()
    assert keys == 110 and flags == 0
    OC = 1 << 16
    wm = api.WorldMap(ctx, km, OC)
    winfo = wm.fuse_torch(cell=1.0, min_count=1, keep="first")
    mo = km.offs.cpu().numpy()
    ms = int(np.diff(mo[:111]).max())
    ml = api.MapLocalizer(ctx, wm, 1.0, 4, ms)
    iinfo = ml.index_torch()
    torch.cuda.synchronize()
    R = int(winfo.cpu()[0])
    assert iinfo.cpu().numpy().tolist() == [R, R, 0, 0] and 1000 < R < OC
    xyz, row = wm.xyz.cpu().numpy()[:R], wm.row.cpu().numpy()[:R]
    ix = mnp.index(xyz, R, 1.0)
    mx, mp = km.xyz.cpu().numpy(), km.poses.cpu().numpy()
    c = len(DRIVE_ROWS)
    pert = np.zeros((c, 3, 4))
    axes = np.array([(0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1)], np.float64)
    for p in range(c):
        a = axes[p] / np.linalg.norm(axes[p])
        pert[p, :, :3] = pg.exp_so3(a * np.deg2rad(1.0)); pert[p, :, 3] = 0.3 * a[[1, 2, 0]]
    idx = dev(DRIVE_ROWS, np.int32)
    kw = dict(max_iter=30, max_corr=0.9, tol_rmse=1e-6, tol_fitness=1e-6, min_inliers=3)
    wT0, wps = mnp.seed(mp, 110, DRIVE_ROWS, None, pert, DRIVE_ROWS)
    truth = np.stack([pg.inv(mp[r].reshape(3, 4)) for r in DRIVE_ROWS])
    for excl in (None, [[r, r] for r in DRIVE_ROWS]):
        T, stats, acc = ml.localize_torch(km.xyz, km.offs, km.poses, km.state, idx, T_rel=dev(pert), src=idx,
                                          excl=None if excl is None else dev(excl, np.int32), min_fitness=0.6, max_rmse=0.5, **kw)
        torch.cuda.synchronize()
        T0, ps = (t.cpu().numpy() for t in ml.last_localize["seed"])
        assert T0.tobytes() == wT0.tobytes() and ps.tolist() == list(DRIVE_ROWS)
        T, stats, acc = T.cpu().numpy(), stats_host(stats), acc.cpu().numpy()
        for p, r in enumerate(DRIVE_ROWS):
            want = mnp.icp(ix, xyz, row, mx[mo[r]:mo[r + 1]], wT0[p], None if excl is None else tuple(excl[p]), **kw)
            before, after = np.abs(wT0[p] - truth[p]).max(), np.abs(T[p] - truth[p]).max()
            print("   row %3d %s: %d points, seed error %.3g -> %.3g, fitness %.3f rmse %.3g iters %d status %d (restated: %.3f %.3g %d %d)"
                  % (r, "own rows excluded" if excl else "no exclusion", mo[r + 1] - mo[r], before, after, stats[p]["fitness"], stats[p]["rmse"],
                     stats[p]["iters"], stats[p]["status"], want["fitness"], want["rmse"], want["iters"], want["status"]))
            assert_refine_matches((T[p], stats[p]), want, (r, excl is not None))
            assert bool(acc[p]) == mnp.accept(want, 0.6, 0.5), (r, excl is not None)
            assert after < before, (r, excl is not None, before, after)
    ml.close(); wm.close(); km.close(); win.close(); ctx.close()
