"""The world map on the device (pr_worldmap, worldmap.hip): every fuse equals the NumPy restatement (worldmap_np.py) BIT FOR
BIT - xyz, inten, src, row, count, state and info - at the launch geometry's edges, under contention and hash collisions, at the rule's
edges, with guard words behind all six buffers and guard values in every row a fuse must not write; the host form, two eager runs and
one captured graph replayed over a growing map give the same bytes; the seq07 drive fused under the map's, the relaxed and the identity
poses; and write_ply round-trips."""
import numpy as np
import pytest
import torch

import posegraph_np as pg
import worldmap_np as wnp
from so_dso_place_recognition_amd import _lib, api
from so_dso_place_recognition_amd.matcher import _stream_context
from test_gpu_map import KCAP, MAXC, PCAP, dev, pose_inputs, same_bytes, seq07  # noqa: F401  (seq07: the drive's fixture)

pytestmark = pytest.mark.gpu

GUARD = -7
ROWS = ("xyz", "inten", "src", "row", "count")
NEVER = 1 << 30                                        # a min_count above every count
I32 = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")


def guarded_world(ctx, km, ocap):
    """a world map over buffers 8 rows (state: 4 words) longer than stated; refill() puts the guard pattern into every row AND the excess"""
    shapes = dict(xyz=(ocap * 3, 24, torch.float64), inten=(ocap, 8, torch.float32), src=(ocap, 8, torch.int64), row=(ocap, 8, torch.int32),
                  count=(ocap, 8, torch.int32), state=(4, 4, torch.int32))
    big = {n: torch.full((used + extra,), GUARD, dtype=dt, device="cuda") for n, (used, extra, dt) in shapes.items()}
    bufs = {n: big[n][:shapes[n][0]] for n in shapes}
    bufs["xyz"] = bufs["xyz"].view(ocap, 3)
    wm = api.WorldMap(ctx, km, ocap, buffers=bufs)

    def refill():
        for n in ROWS:
            big[n].fill_(GUARD)

    def intact():
        for n, (used, extra, dt) in shapes.items():
            assert bool((big[n][used:] == GUARD).all()), n
    return wm, refill, intact


def host_map(km):
    torch.cuda.synchronize()
    return km.xyz.cpu().numpy(), km.inten.cpu().numpy(), km.offs.cpu().numpy()


def snapshot(wm, info):
    torch.cuda.synchronize()
    return {**{n: getattr(wm, n).cpu().numpy().copy() for n in api.WorldMap.NAMES}, "info": info.cpu().numpy().copy()}


def assert_equals(got, want, what):
    """the written rows, state and info equal the restatement's bytes; every row behind them still holds the guard value"""
    r = int(want["state"][0])
    assert same_bytes(got["state"], want["state"]), (what, got["state"], want["state"])
    assert same_bytes(got["info"], want["info"]), (what, got["info"], want["info"])
    for n in ROWS:
        assert same_bytes(got[n][:r], want[n]), (what, n)
        assert (got[n][r:] == GUARD).all(), (what, n, "rows behind the written ones")


def fuse_and_check(wm, refill, intact, km, poses_dev, n_dev, cell, min_count, keep, what):
    """one device fuse against the restatement run on the map's and the pose array's device bytes"""
    refill()
    info = wm.fuse_torch(poses=poses_dev, n=n_dev, cell=cell, min_count=min_count, keep=keep)
    got = snapshot(wm, info)
    xyz, inten, offs = host_map(km)
    poses = (km.poses if poses_dev is None else poses_dev).cpu().numpy()
    n = int((km.state if n_dev is None else n_dev).cpu().numpy()[0])
    want = wnp.fuse(xyz, inten, offs, poses, n, cell, min_count, keep, out_capacity=wm.out_capacity)
    assert_equals(got, want, what)
    intact()
    return got, want


def append(km, x, it=None, pose=None):
    x = np.asarray(x, np.float64).reshape(-1, 3)
    it = np.arange(len(x), dtype=np.float32) * 0.5 if it is None else it
    pose = wnp.identity_poses(1) if pose is None else pose
    return km.append(x, it, np.array([0, len(x)], np.int64), np.zeros((1, 16)), poses=np.asarray(pose).reshape(1, 12), ids=[0])


def rand_pose(rng):
    P = np.zeros((3, 4))
    P[:, :3] = pg.exp_so3(rng.normal(0.0, 1.0, 3))
    P[:, 3] = rng.normal(0.0, 2.0, 3)
    return P.reshape(12)


# ------------------------------------------------------------------------------------------------ 1. launch geometry
# point_capacity -> (max_cloud_points, the cloud sizes of each map; a size above max_cloud_points is a DROPPED row, 0 an empty one)
GEOMETRY = {
    32: (20, [[], [1], [2], [1, 1], [16, 0, 16], [10, 25, 5], [0, 0, 2]]),
    600: (300, [[255], [256], [200, 57], [256, 0, 257], [300, 301, 213], [300, 300], [257, 0, 0]]),
}


@pytest.mark.parametrize("pcap", list(GEOMETRY))
def test_geometry_edges_equal_the_restatement(pcap):
    """0, 1, 2 and 32 points in a table of T = 64 slots, 255, 256, 257, 513 and 600 in one of T = 2048, in 0 .. 3 keyframes with an empty
    row between two full ones and a dropped row; each under both keep values and min_count 1, 2, 3 and one above every count."""
    maxc, maps = GEOMETRY[pcap]
    assert 1 << wnp.log2T(pcap) == (64 if pcap == 32 else 2048)
    ctx = _stream_context(0)
    km = api.KeyframeMap(ctx, 4, pcap, maxc)
    wm, refill, intact = guarded_world(ctx, km, pcap)
    rng = np.random.default_rng(pcap)
    for sizes in maps:
        km.reset()
        for s in sizes:
            info = append(km, rng.normal(0, 0.8, (s, 3)), rng.random(s).astype(np.float32), rand_pose(rng))
            assert bool(info[3] & _lib.MAP_DROPPED) == (s > maxc)
        stored = sum(s for s in sizes if s <= maxc)
        assert km.count()[:2] == (len(sizes), stored)
        for keep in ("first", "last"):
            for mc in (1, 2, 3, NEVER):
                got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.5, mc, keep, (sizes, keep, mc))
                assert want["info"][2] == stored and (mc == 1 or stored < 3 or want["info"][1] < want["info"][2])
                assert mc != NEVER or (want["state"].tolist() == [0, 0, 0, 0] and want["info"].tolist() == [0, 0, stored, 0])
    wm.close(); km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. contention and collisions
def test_one_voxel_own_voxels_and_colliding_keys():
    ctx = _stream_context(0)
    km = api.KeyframeMap(ctx, 4, 600, 300)
    wm, refill, intact = guarded_world(ctx, km, 600)
    rng = np.random.default_rng(3)
    append(km, 0.1 + 0.05 * rng.random((300, 3)))                      # every point in the voxel (0, 0, 0) of cell 0.2: 600 adds on one slot
    append(km, 0.1 + 0.05 * rng.random((300, 3)))
    for keep, rep in (("first", 0), ("last", 599)):
        got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.2, 1, keep, ("one voxel", keep))
        assert want["info"].tolist() == [1, 1, 600, 0] and got["src"][0] == rep and got["count"][0] == 600 and got["row"][0] == rep // 300
        fuse_and_check(wm, refill, intact, km, None, None, 0.2, 600, keep, ("one voxel, min_count = count", keep))
        got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.2, 601, keep, ("one voxel, min_count above", keep))
        assert want["info"].tolist() == [0, 0, 600, 0]
    km.reset()
    grid = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(6), indexing="ij"), -1).reshape(-1, 3) - 4.0   # 600 cells
    grid = grid[rng.permutation(600)]
    append(km, (grid[:300] + 0.5) * 0.25); append(km, (grid[300:] + 0.5) * 0.25)
    for keep in ("first", "last"):
        got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.25, 1, keep, ("own voxels", keep))
        assert want["info"].tolist() == [600, 600, 600, 0] and got["src"].tolist() == list(range(600)) and (got["count"] == 1).all()
    wm.close(); km.close()
    # T = 64: 32 distinct keys, ten of them with the home slot 62 - their chain runs 62, 63, 0, 1, ... (asserted in test_worldmap_cpu.py)
    km = api.KeyframeMap(ctx, 4, 32, 32)
    wm, refill, intact = guarded_world(ctx, km, 32)
    cells = np.array(wnp.COLLIDING_CELLS, np.float64)
    append(km, cells[:20] + 0.5); append(km, cells[20:] + 0.5)
    got, want = fuse_and_check(wm, refill, intact, km, None, None, 1.0, 1, "first", "colliding keys")
    assert want["info"].tolist() == [32, 32, 32, 0] and want["keys"] == set(wnp.COLLIDING_CELLS)
    km.reset()                                                          # each colliding key twice: first and last differ in every row
    append(km, cells[:16] + 0.5); append(km, cells[:16] + 0.25)
    for keep in ("first", "last"):
        got, want = fuse_and_check(wm, refill, intact, km, None, None, 1.0, 2, keep, ("colliding keys twice", keep))
        assert want["info"].tolist() == [16, 16, 32, 0] and (got["count"][:16] == 2).all() and (got["row"][:16] == (keep == "last")).all()
    wm.close(); km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the rule's edges
def test_rule_edges():
    ctx = _stream_context(0)
    kcap, pcap = 4, 600
    km = api.KeyframeMap(ctx, kcap, pcap, 300)
    wm, refill, intact = guarded_world(ctx, km, pcap)
    rng = np.random.default_rng(4)
    lim = float(1 << 20)
    edge = np.zeros((12, 3))
    edge[0] = (lim, 0, 0); edge[1] = (lim - 1, 0, 0); edge[2] = (-lim, 0, 0); edge[3] = (0, np.nextafter(lim, 0), 0); edge[4] = (0, 0, -lim - 1)
    edge[5] = (np.nan, 1, 1); edge[6] = (-0.0, -0.0, -0.0); edge[7] = (0.0, -0.0, 0.0); edge[8] = (2, np.inf, 2); edge[9] = (-1e-300, 0, 0)
    edge[10] = (3.0, 3.0, 3.0); edge[11] = (-3.0, -3.0, -3.0)
    append(km, edge)                                                    # row 0: the identity pose, cell = 1
    sizes = (12, 200, 150, 100)                                         # the map is full: 4 keyframes; the random clouds lie > 100 m from row 0's
    for s in sizes[1:]:
        append(km, rng.normal(0, 2, (s, 3)) + 100.0, pose=rand_pose(rng))
    got, want = fuse_and_check(wm, refill, intact, km, None, None, 1.0, 1, "first", "range, NaN point, -0.0")
    assert want["info"][3] == wnp.SKIPPED | wnp.RANGE and want["info"][2] == 12 - 4 + 450
    assert got["src"][:7].tolist() == [1, 2, 3, 6, 9, 10, 11] and got["count"][3] == 2        # 2^20 - 1 and -2^20 kept; the two zeros share a voxel
    assert np.signbit(got["xyz"][3]).tolist() == [True, True, True] and got["xyz"][3].tolist() == [0.0, 0.0, 0.0]   # -0.0 keeps its sign
    got, want = fuse_and_check(wm, refill, intact, km, None, None, 1.0, 1, "last", "range, NaN point, -0.0 / last")
    assert got["src"][3] == 7 and np.signbit(got["xyz"][3]).tolist() == [False, False, False]
    # a NaN and an Inf in a pose row: every point of that row is skipped, the others are not touched
    for row, word, bad in ((1, 5, np.nan), (2, 11, np.inf), (1, 0, -np.inf)):
        poses = km.poses.clone()
        poses[row, word] = bad
        got, want = fuse_and_check(wm, refill, intact, km, poses, None, 1.0, 1, "first", ("pose", row, word, bad))
        assert want["info"][3] & wnp.SKIPPED and not (got["row"][:int(want["state"][0])] == row).any()
        assert want["info"][2] == 8 + 450 - sizes[row]
    # d_n: above keyframe_capacity (clamped to it), below zero, a count below the map's, and a scribbled state word of the map
    for n, rows_seen in ((99, 4), (kcap + 1, 4), (-5, 0), (0, 0), (1, 1), (2, 2)):
        got, want = fuse_and_check(wm, refill, intact, km, None, I32(n), 0.5, 1, "first", ("n", n))
        assert len(set(got["row"][:int(want["state"][0])].tolist())) == rows_seen
        assert n > 0 or want["info"].tolist() == [0, 0, 0, 0]
    keep_state = km.state.clone()
    for scribble in (1 << 30, -3):
        km.state[0] = scribble
        got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.5, 2, "last", ("scribbled state", scribble))
        assert (want["info"][2] > 0) == (scribble > 0)
    km.state.copy_(keep_state)
    wm.close()
    # out_capacity below the qualifying count: OVERFLOW, the tail keeps its guard values, info[1] is the true count
    wm, refill, intact = guarded_world(ctx, km, 40)
    for keep in ("first", "last"):
        got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.5, 1, keep, ("overflow", keep))
        assert want["info"][0] == 40 < want["info"][1] and want["info"][3] & wnp.OVERFLOW and got["state"].tolist() == [40, int(want["info"][3]), 0, 0]
        full = wnp.fuse(*host_map(km), km.poses.cpu().numpy(), 4, 0.5, 1, keep)
        assert same_bytes(full["src"][:40], got["src"]) and full["info"][1] == want["info"][1] and not full["info"][3] & wnp.OVERFLOW
    got, want = fuse_and_check(wm, refill, intact, km, None, None, 0.5, 3, "first", "no overflow at min_count 3")
    assert want["info"][1] <= 40 and not want["info"][3] & wnp.OVERFLOW                      # the flag is the call's: nothing is sticky
    wm.close(); km.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the forms
def test_host_form_two_runs_and_one_graph_over_a_growing_map():
    rng = np.random.default_rng(5)
    clouds = [(rng.normal(0, 1.0, (s, 3)), rng.random(s).astype(np.float32), rand_pose(rng)) for s in (257, 300, 43)]
    relaxed = np.stack([rand_pose(rng) for _ in range(4)])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, 4, 600, 300)
        wm, refill, intact = guarded_world(ctx, km, 600)
        poses = dev(relaxed)
        info = torch.zeros(4, dtype=torch.int64, device="cuda")
        args = dict(poses=poses, cell=0.5, min_count=2, keep="last")
        wm.fuse_torch(info=info, **args)                                # eager once (the empty map), then the capture - on the empty map
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            wm.fuse_torch(info=info, **args)
        for count in range(4):
            if count:
                append(km, *clouds[count - 1])
            xyz, inten, offs = host_map(km)
            want = wnp.fuse(xyz, inten, offs, relaxed, count, 0.5, 2, "last")
            assert (count == 0) == (want["info"][1] == 0)
            refill(); info.fill_(GUARD)
            g.replay()
            replayed = snapshot(wm, info)
            assert_equals(replayed, want, ("replayed", count))
            runs = []
            for _ in range(2):
                refill(); info.fill_(GUARD)
                wm.fuse_torch(info=info, **args)
                runs.append(snapshot(wm, info))
            for n in runs[0]:
                assert same_bytes(runs[0][n], runs[1][n]) and same_bytes(runs[0][n], replayed[n]), (count, n)
            intact()
            refill()
            hx, hi, hs, hr, hc, hinfo = wm.fuse(poses=relaxed, n=count, cell=0.5, min_count=2, keep="last")      # the host form
            host = dict(xyz=hx, inten=hi, src=hs, row=hr, count=hc)
            assert same_bytes(hinfo, want["info"]) and all(same_bytes(host[n], want[n]) for n in ROWS), count
            assert wm.count_rows() == (int(want["state"][0]), int(want["state"][1]))
            hx2 = wm.fuse(cell=0.5, min_count=1)                          # NULL poses and n: the map's own
            own = wnp.fuse(xyz, inten, offs, km.poses.cpu().numpy(), count, 0.5, 1, "first")
            assert same_bytes(hx2[0], own["xyz"]) and same_bytes(hx2[5], own["info"]), count
        del g
        wm.close(); km.close(); ctx.close()


def test_live_handle_refusals():
    ctx, other = _stream_context(0), _stream_context(0)
    km = api.KeyframeMap(other, 4, 64, 16)
    with pytest.raises(ValueError, match="share one context"):
        api.WorldMap(ctx, km, 8)
    lib = ctx.lib
    rec = _lib.WorldMapBuffers(*([km.state.data_ptr()] * 6))           # never written: the create below is refused
    import ctypes as C
    h = C.c_void_p()
    assert lib.pr_worldmap_create(ctx.h, km.h, C.byref(rec), 8, C.byref(h)) == _lib.PR_EINVAL and not h.value
    assert b"another context" in lib.pr_last_error(ctx.h)
    wm = api.WorldMap(other, km, 8)
    with pytest.raises(_lib.PRError, match="d_info is NULL"):
        other.check(lib.pr_worldmap_fuse_dev(wm.h, None, None, 0.2, 1, 0, None))
    with pytest.raises(_lib.PRError, match="cell must be finite and positive"):
        wm.fuse_torch(cell=0.0)
    with pytest.raises(_lib.PRError, match="min_count=0"):
        wm.fuse(min_count=0)
    wm.close(); km.close(); other.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the drive
def test_the_drive_fused_under_the_maps_the_relaxed_and_the_identity_poses(seq07):
    """The seq07 drive of test_gpu_map.py (60 points per pose, 110 keyframes) through push_torch -> append_push, then fused under the
    map's own poses, the poses relax_map returns for a log of three closures, and the identity for every row."""
    ctx = _stream_context(0)
    win = api.CloudWindow(ctx, 45.0, False, 9000, 60, 9000)
    km = api.KeyframeMap(ctx, KCAP, PCAP, MAXC)
    out = win.empty_out()
    for p in range(len(seq07["pid"])):
        w, x, it, k, pid = pose_inputs(seq07, p)
        win.push_torch(dev(w), dev(x), dev(it, np.float32), I32(k), out=out)
        km.append_push(out, pose=dev(w), id=I32(pid))
    keys, points, flags = km.count()
    assert keys == 110 and flags == 0 and points > 10000
    graph = api.PoseGraph(ctx, KCAP, 8)
    P = km.poses.cpu().numpy().reshape(KCAP, 3, 4)
    for i, j in ((2, 100), (10, 90), (30, 109)):                        # closures that disagree with the odometry by 0.3 m
        Z = pg.mul(P[i], pg.inv(P[j]))
        Z[:, 3] += (0.3, -0.2, 0.1)
        graph.add([i], Z.reshape(1, 12), [1], j, 100.0, 10.0)
    corrected = torch.zeros((KCAP, 12), dtype=torch.float64, device="cuda")
    graph.relax_map(km, out=corrected, outer=3, inner=32, lam=1e-9, w_odo_rot=100.0, w_odo_trans=10.0)
    torch.cuda.synchronize()
    moved = np.abs(corrected.cpu().numpy()[:110] - P.reshape(KCAP, 12)[:110]).max()
    assert 0.01 < moved < 1.0, moved
    OC = 1 << 16
    wm, refill, intact = guarded_world(ctx, km, OC)
    ident = dev(wnp.identity_poses(KCAP))
    seen = {}
    for name, poses in (("map", None), ("relaxed", corrected), ("identity", ident)):
        got, want = fuse_and_check(wm, refill, intact, km, poses, None, 0.2, 2, "first", name)
        seen[name] = want["info"].tolist()
        print("   the drive under the", name, "poses:", points, "points ->", seen[name])
        assert want["info"][2] == points and want["info"][3] in (0, wnp.OVERFLOW) and want["info"][1] > 100
    assert seen["map"] != seen["identity"]                              # camera-frame clouds pile up around the origin
    fuse_and_check(wm, refill, intact, km, corrected, None, 1.0, 1, "last", "relaxed, cell 1.0, last")
    wm.close(); graph.close(); km.close(); win.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 6. write_ply
def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    names = [l.split()[2] for l in lines if l.startswith("property")]
    dt = np.dtype([(l.split()[2], {"double": "<f8", "float": "<f4", "int": "<i4"}[l.split()[1]]) for l in lines if l.startswith("property")])
    if "binary_little_endian" in lines[1]:
        return names, np.frombuffer(body, dt, n)
    rows = [l.split() for l in body.decode("ascii").split("\n") if l]
    return names, np.array([tuple(float(v) for v in r) for r in rows], dt) if n else np.zeros(0, dt)


@pytest.mark.parametrize("binary", [True, False])
def test_write_ply_round_trips(tmp_path, binary):
    ctx = _stream_context(0)
    km = api.KeyframeMap(ctx, 4, 600, 300)
    rng = np.random.default_rng(6)
    append(km, rng.normal(0, 1.0, (300, 3)), rng.random(300).astype(np.float32), rand_pose(rng))
    append(km, rng.normal(0, 1.0, (200, 3)), rng.random(200).astype(np.float32), rand_pose(rng))
    wm = api.WorldMap(ctx, km, 600)
    info = wm.fuse_torch(cell=0.5, min_count=1)
    path = str(tmp_path / "world.ply")
    r = wm.write_ply(path, binary=binary)
    names, v = read_ply(path)
    xyz, inten, src, row, count = wm.rows()
    assert names == ["x", "y", "z", "intensity", "count"] and r == len(v) == int(info.cpu()[0]) == len(src) and 50 < r < 500
    assert same_bytes(np.stack([v["x"], v["y"], v["z"]], 1), xyz) and same_bytes(v["intensity"].copy(), inten) and same_bytes(v["count"].copy(), count)
    wm.close(); km.close(); ctx.close()
