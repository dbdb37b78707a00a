"""Snapshots on the device (pr_snapshot) against the NumPy restatement tests/snapshot_np.py: the packed blob byte for
byte, the unpacked buffers byte for byte (equal and larger destinations), every refusal decided on the device with the destination left
untouched, the file round trip into a fresh process, and the contract that matters: a drive interrupted by save -> destroy -> create
larger -> load continues to the same bytes as the uninterrupted run (the seq07 scene and the two-drive scene of test_gpu_session.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import session_np as sn
import snapshot_child
import snapshot_np as sp
from snapshot_rig import GUARD_BYTE, Rig, seq07_batch_clouds
from so_dso_place_recognition_amd import _lib, api, graph
from so_dso_place_recognition_amd.matcher import _stream_context
from so_dso_place_recognition_amd.snapshot import Snapshot

pytestmark = pytest.mark.gpu

# the capacities of the pack cases: 258 keyframes hold the 257-row case with a row to spare, clouds up to 513 points
FULL = dict(map=(258, 40000, 513), online=(("sc", 258), ("m2dp", 258)), set=("fused", 5), graphs=(600, 600), sessions=4, nodes=258)
CLOUDS = (1, 0, 64, 513, 7, 0)          # cycled over the rows: an empty row and (zero frame) a dropped one among them
# (map rows, online rows x 2, set rows, edges x 2, sessions)
CASES = {"empty": (0, 0, 0, 0, 0, 0, 1), "one": (1, 1, 1, 1, 1, 0, 2), "63": (63, 257, 0, 3, 513, 1, 4), "64": (64, 0, 257, 5, 0, 513, 1),
         "65": (65, 1, 257, 2, 513, 513, 3), "257": (257, 257, 257, 5, 600, 7, 4)}
SMALL = dict(map=(8, 64, 16), online=(("sc", 4), ("m2dp", 4)), set=("fused", 3), graphs=(4, 4), sessions=4, nodes=8)
SMALL_COUNTS = (5, 3, 2, 2, 3, 1, 3)
SMALL_CLOUDS = (3, 0, 16, 1, 7)


def filled(spec, counts, seed, clouds=CLOUDS):
    from snapshot_rig import spec_state
    st = spec_state(spec)
    for k, (part, n) in enumerate(zip(st, counts)):
        sizes = [clouds[i % len(clouds)] for i in range(n)] if part["kind"] == sp.MAP else None
        sp.fill(part, seed * 32 + k, n, cloud_sizes=sizes)
    return st


def check_pack(rig, state, what, capacity=None):
    """the device's blob and info against the restatement's; the bytes behind what was written keep the guard pattern"""
    want, winfo = sp.pack(state, blob_capacity=capacity)
    raw, info = rig.pack(capacity)
    assert info.tolist() == winfo.tolist(), (what, info, winfo)
    assert raw[:want.size].tobytes() == want.tobytes(), (what, "the blob", int(np.flatnonzero(raw[:want.size] != want)[0]))
    assert (raw[want.size:] == GUARD_BYTE).all(), (what, "a byte behind the written extent")
    rig.intact()
    return want, info


@pytest.fixture(scope="module")
def full():
    rig = Rig(FULL)
    yield rig
    rig.close()


# ------------------------------------------------------------------------------------------------ 1. pack
@pytest.mark.parametrize("name", list(CASES))
def test_pack_equals_the_restatement_all_parts_together(full, name):
    state = filled(FULL, CASES[name], 1 + list(CASES).index(name))
    full.upload(state)
    want, info = check_pack(full, state, name)
    again, _ = full.pack()
    assert again[:want.size].tobytes() == want.tobytes()                              # two runs give the same bytes
    assert sp.state_bytes(full.download()) == sp.state_bytes(state)                   # the pack only reads
    assert info[0] <= full.snap.bound() == sp.bound(state) and sp.validate(state, want)[0].tolist() == [17, -1, 0, 0]


ALONE = {"map": dict(map=(66, 3000, 513)), "sc": dict(online=(("sc", 3),)), "m2dp": dict(online=(("m2dp", 3),)), "fused": dict(set=("fused", 3)),
         "delight": dict(set=("delight", 3)), "log": dict(graphs=(5,)), "two_logs": dict(graphs=(5, 9)), "sessions": dict(sessions=4)}


@pytest.mark.parametrize("name", list(ALONE))
def test_pack_and_unpack_every_part_alone(name):
    spec = ALONE[name]
    rig, dst = Rig(spec), Rig(spec)
    for n in (0, 1, 3):
        counts = [n * 7 if name == "map" else n] * len(rig.model)
        state = filled(spec, counts, 40 + n)
        rig.upload(state)
        want, info = check_pack(rig, state, (name, n))
        dst.fill_bytes(0x5C)
        before = dst.download()
        winfo = sp.unpack(before, want)
        assert dst.unpack(want).tolist() == winfo.tolist() == [len(sp.sections(state)), -1, 0, 0], (name, n)
        assert sp.state_bytes(dst.download()) == sp.state_bytes(before), (name, n)
        dst.intact()
    rig.close(); dst.close()


@pytest.mark.parametrize("what", ["negative", "above", "offs_above", "offs_negative"])
def test_scribbled_counts_are_clamped_before_they_form_an_address(full, what):
    state = filled(FULL, CASES["65"], 9)
    for part in state:
        if what == "negative":
            part["state"][0] = -3
        elif what == "above":
            part["state"][0] = 1 << 30
    if what.startswith("offs"):
        state[0]["arrays"]["offs"][65] = (1 << 40) if what == "offs_above" else -5
    full.upload(state)
    want, info = check_pack(full, state, what)
    d = sp.describe(want)
    if what == "above":
        assert [e["rows"] for e in d["table"]] == [0, 0, 259, 258, 258, 258, 258, 258, 5, 5, 600, 600, 600, 600, 600, 600, 4]     # offs[258] = 0
    if what == "negative":
        assert [e["rows"] for e in d["table"]] == [0, 0, 1] + [0] * 13 + [1] and d["table"][0]["state"][0] == -3
    if what.startswith("offs"):
        assert d["table"][0]["rows"] == (40000 if what == "offs_above" else 0)


def test_a_blob_that_does_not_fit(full):
    state = filled(FULL, CASES["63"], 5)
    full.upload(state)
    whole, info = check_pack(full, state, "whole")
    ext = 64 + 128 * 17
    for cap in (int(info[0]) - 1, int(info[0]) - 16, ext, ext - 16, 16):
        head, hinfo = check_pack(full, state, ("capacity", cap), capacity=cap)       # guard words behind the header (or behind nothing) untouched
        assert hinfo.tolist() == [int(info[0]), 17, sp.OVERFLOW, 0] and head.size == (ext if cap >= ext else 0)
    exact, einfo = check_pack(full, state, "exact", capacity=int(info[0]))
    assert einfo[2] == 0 and exact.tobytes() == whole.tobytes()


def test_one_capture_on_empty_state_replayed_at_three_counts():
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rig = Rig(FULL)
        rig.upload(filled(FULL, CASES["empty"], 3))
        cap = rig.snap.bound()
        blob = rig.blob(cap)
        info = torch.zeros(4, dtype=torch.int64, device="cuda")
        rig.snap.pack_torch(blob[:cap], info=info)       # one eager call, then the capture of the same call
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            rig.snap.pack_torch(blob[:cap], info=info)
        for name in ("one", "65", "257"):
            state = filled(FULL, CASES[name], 20 + len(name))
            rig.upload(state)
            blob.fill_(GUARD_BYTE); info.fill_(-1)
            g.replay()
            st.synchronize()
            got, ginfo = blob.cpu().numpy(), info.cpu().numpy()
            eager, einfo = rig.pack()
            want, winfo = sp.pack(state)
            assert ginfo.tolist() == einfo.tolist() == winfo.tolist(), name
            assert got[:want.size].tobytes() == eager[:want.size].tobytes() == want.tobytes() and (got[want.size:] == GUARD_BYTE).all(), name
        del g
        rig.close()


def test_buffers_off_a_16_byte_boundary():
    """caller buffers that are only as aligned as their element type: the lanes fall back to 4-byte loads and stores, the bytes are the same"""
    ctx = _stream_context(0)
    ec, sc, GI = 7, 4, -7

    def make():
        big = dict(edge_ij=torch.full((2 * ec + 8,), GI, dtype=torch.int32, device="cuda"), edge_Z=torch.full((12 * ec + 8,), -7.0, dtype=torch.float64, device="cuda"),
                   edge_w=torch.full((2 * ec + 8,), -7.0, dtype=torch.float64, device="cuda"), state=torch.full((12,), GI, dtype=torch.int32, device="cuda"),
                   start=torch.full((sc + 8,), GI, dtype=torch.int32, device="cuda"), sstate=torch.full((12,), GI, dtype=torch.int32, device="cuda"))
        g = api.PoseGraph(ctx, 8, ec, buffers=dict(edge_ij=big["edge_ij"][2:2 + 2 * ec].view(ec, 2), edge_Z=big["edge_Z"][1:1 + 12 * ec].view(ec, 12),
                                                   edge_w=big["edge_w"][1:1 + 2 * ec].view(ec, 2), state=big["state"][1:5]))
        t = graph.SessionTable(ctx, 8, ec, sc, buffers=dict(start=big["start"][1:1 + sc], state=big["sstate"][3:7]))
        assert g.edge_ij.data_ptr() % 16 == 8 and g.edge_Z.data_ptr() % 16 == 8 and t.start.data_ptr() % 16 == 4
        return big, g, t, Snapshot(ctx, graphs=(g,), sessions=t)

    spec = dict(graphs=(ec,), sessions=sc)
    state = filled(spec, (5, 3), 12)
    big, g, t, snap = make()
    for nm in api.PoseGraph.NAMES:
        getattr(g, nm).copy_(dev(state[0]["state"] if nm == "state" else state[0]["arrays"][nm], state[0]["state"].dtype if nm == "state" else state[0]["arrays"][nm].dtype))
    t.start.copy_(dev(state[1]["arrays"]["start"], np.int32)); t.state.copy_(dev(state[1]["state"], np.int32))
    want, winfo = sp.pack(state)
    blob = torch.full((snap.bound() + 64,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    info = snap.pack_torch(blob[:snap.bound()])
    ctx.sync()
    assert info.cpu().tolist() == winfo.tolist() and blob.cpu().numpy()[:want.size].tobytes() == want.tobytes()
    assert bool((blob[want.size:] == GUARD_BYTE).all())
    big2, g2, t2, snap2 = make()
    assert snap2.unpack_torch(blob[:want.size]).cpu().tolist() == [4, -1, 0, 0]
    ctx.sync()
    for a, b in ((g, g2), (t, t2)):
        for nm in a.NAMES:
            x, y = getattr(a, nm).cpu().numpy(), getattr(b, nm).cpu().numpy()
            rows = {"edge_ij": 5, "edge_Z": 5, "edge_w": 5, "start": 3, "state": 4}[nm]
            assert same_bytes(x[:rows], y[:rows]), nm
    for k, v in big2.items():                            # rows above the counts and the guards around the views keep their fill
        lo, used = {"edge_ij": (2, 10), "edge_Z": (1, 60), "edge_w": (1, 10), "state": (1, 4), "start": (1, 3), "sstate": (3, 4)}[k]
        h = v.cpu().numpy()
        assert (h[:lo] == -7).all() and (h[lo + used:] == -7).all(), k
    snap.close(); snap2.close(); t.close(); t2.close(); g.close(); g2.close(); ctx.close()


# ------------------------------------------------------------------------------------------------ 2. unpack
def grown(spec, kf=lambda c: c, pts=1, edges=1):
    kc, pc, mcp = spec["map"]
    return dict(spec, map=(kf(kc), pc * pts, mcp), graphs=tuple(c * edges for c in spec["graphs"]), nodes=kf(spec["nodes"]))


@pytest.mark.parametrize("dest", ["equal", "keyframes+1", "x2"])
def test_unpack_into_equal_and_larger_destinations(full, dest):
    spec = {"equal": FULL, "keyframes+1": grown(FULL, kf=lambda c: c + 1), "x2": grown(FULL, kf=lambda c: 2 * c, pts=2, edges=2)}[dest]
    dst = Rig(spec)
    for name in ("empty", "65", "257"):
        state = filled(FULL, CASES[name], 60 + len(name))
        blob, _ = sp.pack(state)
        dst.fill_bytes(0x5C)
        before = dst.download()
        assert sp.unpack(before, blob).tolist() == [17, -1, 0, 0]
        assert dst.unpack(blob).tolist() == [17, -1, 0, 0], (dest, name)
        after = dst.download()
        # rows below the counts and every state as saved, rows at and above them as the destination held them: the restatement's bytes
        assert sp.state_bytes(after) == sp.state_bytes(before), (dest, name)
        dst.intact()
        again, ainfo = check_pack(dst, after, (dest, name, "unpack then pack"))
        if dest == "equal":
            assert again.tobytes() == blob.tobytes()                                  # the original blob again
        else:
            ext = 64 + 128 * 17
            assert again[ext:].tobytes() == blob[ext:].tobytes()                      # the sections; the table records the new capacities
            da, db = sp.describe(again), sp.describe(blob)
            keys = ("kind", "subtype", "array", "rows", "row_bytes", "offset", "length", "checksum", "state")
            assert [[e[k] for k in keys] for e in da["table"]] == [[e[k] for k in keys] for e in db["table"]]
    dst.close()


# ------------------------------------------------------------------------------------------------ 3. refusals decided on the device
def resum(blob, s):
    """the checksum of section s recomputed after an edit of its bytes on purpose, and the table's with it"""
    e = sp.describe(blob)["table"][s]
    blob[64 + 128 * s + 56:64 + 128 * s + 64] = np.array([sp.checksum(blob[e["offset"]:e["offset"] + e["length"]])], np.uint64).view(np.uint8)
    return sp.retable(blob)


def small_blob():
    state = filled(SMALL, SMALL_COUNTS, 77, clouds=SMALL_CLOUDS)
    blob, info = sp.pack(state)
    assert info.tolist() == [blob.size, 17, 0, 0] and all(e["length"] > 0 for e in sp.describe(blob)["table"])
    return state, blob


def refusals():
    state, blob = small_blob()
    d = sp.describe(blob)["table"]
    out = {}
    for s in range(17):                                  # one flipped bit in each section in turn
        b = blob.copy(); b[d[s]["offset"] + d[s]["length"] // 2] ^= 0x10
        out[f"bit_in_section_{s}"] = (b, None, None)
    b = blob.copy(); b[64 + 128 * 7 + 24] ^= 1
    out["count_in_table"] = (b, None, None)
    out["count_in_table_resummed"] = (sp.retable(b.copy()), None, None)
    b = blob.copy(); b[0] ^= 0x20
    out["magic"] = (b, None, None)
    b = blob.copy(); b[8:16] = np.array([sp.VERSION + 1], np.int64).view(np.uint8)
    out["version"] = (b, None, None)
    o = d[2]["offset"]
    b = blob.copy(); b[o + 8:o + 16] = np.array([4], np.int64).view(np.uint8)        # offs = 0 4 3 19 20 27: descending at row 1, no cloud above 16
    out["offs_descending"] = (resum(b, 2), None, None)
    b = blob.copy(); b[o:o + 8] = np.array([1], np.int64).view(np.uint8)
    out["offs_0"] = (resum(b, 2), None, None)
    b = blob.copy(); b[o + 40:o + 48] = np.array([26], np.int64).view(np.uint8)      # offs[keyframes] is not the rows of xyz
    out["offs_end"] = (resum(b, 2), None, None)
    so = d[16]["offset"]
    b = blob.copy(); b[so + 4:so + 8] = 0                                            # start = 0 0 ...: not ascending
    out["session_starts"] = (resum(b, 16), None, None)
    from snapshot_rig import spec_state
    less = [p for p in state if not (p["kind"] == sp.ONLINE and p["subtype"] == sp.TYPE_M2DP)]
    out["a_section_missing"] = (sp.pack(less)[0], None, None)
    swapped = dict(SMALL, online=(("m2dp", 4), ("sc", 4)))
    out["the_other_online_type"] = (sp.pack(filled(swapped, SMALL_COUNTS, 78, clouds=SMALL_CLOUDS))[0], None, None)
    out["cut_inside_the_last_section"] = (blob, d[16]["offset"] + d[16]["length"] - 4, None)
    out["cut_inside_the_table"] = (blob, 64 + 128 * 17 - 8, None)
    out["cut_inside_the_header"] = (blob, 56, None)
    kc, pc, mcp = SMALL["map"]
    out["one_keyframe_too_small"] = (blob, None, dict(SMALL, map=(4, pc, mcp), nodes=4))
    out["one_point_too_small"] = (blob, None, dict(SMALL, map=(kc, 26, mcp)))
    out["a_cloud_above_max_cloud_points"] = (blob, None, dict(SMALL, map=(kc, pc, 15)))
    out["one_signature_too_small"] = (blob, None, dict(SMALL, online=(("sc", 2), ("m2dp", 4))))
    out["one_edge_too_small"] = (blob, None, dict(SMALL, graphs=(2, 4)))
    out["one_session_too_small"] = (blob, None, dict(SMALL, sessions=2))
    return out


REFUSALS = refusals()
EXPECTED_FLAGS = {"magic": sp.BAD_MAGIC, "version": sp.BAD_VERSION, "offs_descending": sp.OFFSETS, "offs_0": sp.OFFSETS, "offs_end": sp.OFFSETS,
                  "session_starts": sp.SESSIONS, "count_in_table": sp.CHECKSUM | sp.TRUNCATED, "count_in_table_resummed": sp.TRUNCATED,
                  "cut_inside_the_last_section": sp.TRUNCATED, "cut_inside_the_table": sp.TRUNCATED, "cut_inside_the_header": sp.TRUNCATED,
                  "one_keyframe_too_small": sp.CAPACITY, "one_point_too_small": sp.CAPACITY, "a_cloud_above_max_cloud_points": sp.CAPACITY,
                  "one_signature_too_small": sp.CAPACITY, "one_edge_too_small": sp.CAPACITY, "one_session_too_small": sp.CAPACITY,
                  "the_other_online_type": sp.MISSING, "a_section_missing": sp.MISSING}
EXPECTED_FIRST = {"magic": -1, "version": -1, "offs_descending": 2, "offs_0": 2, "offs_end": 2, "session_starts": 16, "count_in_table": 7,
                  "count_in_table_resummed": 7, "cut_inside_the_last_section": 16, "cut_inside_the_table": -1, "cut_inside_the_header": -1,
                  "one_keyframe_too_small": 2, "one_point_too_small": 0, "a_cloud_above_max_cloud_points": 2, "one_signature_too_small": 6,
                  "one_edge_too_small": 10, "one_session_too_small": 16, "the_other_online_type": 6, "a_section_missing": 7}


@pytest.fixture(scope="module")
def small():
    rig = Rig(SMALL)
    yield rig
    rig.close()


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refused_blob_changes_no_byte(small, name):
    blob, nbytes, spec = REFUSALS[name]
    dst = small if spec is None else Rig(spec)
    dst.upload(filled(dst.spec, [1] * 7, 90))           # a destination that holds a state of its own
    before = dst.download()
    winfo, _ = sp.validate(before, blob, nbytes)
    if name.startswith("bit_in_section_"):
        assert winfo[0] == 0 and winfo[1] == int(name.rsplit("_", 1)[1]) and winfo[2] & sp.CHECKSUM      # (a flipped offset or start may break its order too)
    else:
        assert winfo[0] == 0 and winfo[1] == EXPECTED_FIRST[name] and winfo[2] == EXPECTED_FLAGS[name], (name, winfo)
    info = dst.unpack(blob, nbytes)
    assert info.tolist() == winfo.tolist(), (name, info, winfo)
    assert sp.state_bytes(dst.download()) == sp.state_bytes(before), (name, "a byte of a destination changed")
    dst.intact()
    if spec is not None:
        dst.close()


def test_the_blob_itself_is_in_order(small):
    state, blob = small_blob()
    small.fill_bytes(0x5C)
    assert small.unpack(blob).tolist() == [17, -1, 0, 0]
    got = small.download()
    assert all(g["state"].tobytes() == s["state"].tobytes() for g, s in zip(got, state))


# ------------------------------------------------------------------------------------------------ 4. the file, across processes
def test_file_round_trip_across_processes(small, tmp_path):
    state = filled(SMALL, SMALL_COUNTS, 31, clouds=SMALL_CLOUDS)
    small.upload(state)
    path = str(tmp_path / "drive.snap")
    small.snap.save(path)
    assert not os.path.exists(path + ".tmp")
    raw, info = small.pack()
    assert open(path, "rb").read() == raw[:int(info[0])].tobytes() == sp.pack(state)[0].tobytes()      # host form = device form = restatement
    want = snapshot_child.digests(state)
    for spec in (SMALL, grown(SMALL, kf=lambda c: 2 * c, pts=2, edges=2)):           # one child at a time
        sj = str(tmp_path / "spec.json")
        json.dump(spec, open(sj, "w"))
        r = subprocess.run([sys.executable, os.path.abspath(snapshot_child.__file__), sj, path], timeout=120, capture_output=True, text=True)
        assert r.returncode == 0, f"the child left with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        got = json.loads(r.stdout.strip().split("\n")[-1])
        assert got["info"] == [17, -1, 0, 0] and got["digests"] == want
        if spec is SMALL:
            import hashlib
            assert got["blob"] == hashlib.sha256(open(path, "rb").read()).hexdigest() and got["pack_info"] == info.tolist()
    # the host form reports what the device decided, and a refused file changes nothing
    bad = bytearray(open(path, "rb").read()); bad[sp.describe(np.frombuffer(bytes(bad), np.uint8))["table"][4]["offset"]] ^= 1
    open(path + ".bad", "wb").write(bytes(bad))
    before = small.download()
    assert small.snap.load(path + ".bad").tolist() == [0, 4, sp.CHECKSUM, 0] and sp.state_bytes(small.download()) == sp.state_bytes(before)
    with pytest.raises(_lib.PRError, match="cannot open"):
        small.snap.load(str(tmp_path / "missing.snap"))
    small.fill_bytes(0x5C)
    exp = small.download()
    sp.unpack(exp, sp.pack(state)[0])
    assert small.snap.load(path).tolist() == [17, -1, 0, 0] and sp.state_bytes(small.download()) == sp.state_bytes(exp)
    small.intact()


# ------------------------------------------------------------------------------------------------ 5. continuation: the two-drive scene
def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def two_drives(c, path):
    """test_gpu_session.py's scene as it would be driven: every row appended to a KeyframeMap (a two-point cloud each), every closure
    logged when its later row exists; begin at row 40; then align -> gate -> relax.  path: drive 1, SAVE, destroy everything, fresh
    handles on a fresh context, LOAD, begin, drive 2; None: uninterrupted."""
    N, EC = c["node_capacity"], c["cap"]
    lg = c["log"]
    E = int(lg.state[0])

    def make():
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, N, 4 * N, 8)
        src, dst = api.PoseGraph(ctx, N, EC), api.PoseGraph(ctx, N, EC)
        table = graph.SessionTable(ctx, N, EC, 4)
        return dict(ctx=ctx, km=km, src=src, dst=dst, table=table, snap=Snapshot(ctx, map=km, graphs=(src, dst), sessions=table))

    def close(h):
        for k in ("snap", "table", "dst", "src", "km", "ctx"):
            h[k].close()

    def drive(h, rows):
        for r in rows:
            x = np.array([[r, 1.0, 2.0], [r, -1.0, 0.5]])
            fr = np.arange(16, dtype=np.float64) + r
            h["km"].append_torch(dev(x), dev([0.25, 0.5], np.float32), dev([0, 2], np.int64), dev(fr), poses=dev(c["poses"][r][None]),
                                 ids=dev([1000 + r], np.int32))
            for e in range(E):
                if max(int(lg.edge_ij[e, 0]), int(lg.edge_ij[e, 1])) == r:
                    h["src"].add([int(lg.edge_ij[e, 0])], lg.edge_Z[e], [1], int(lg.edge_ij[e, 1]), *lg.edge_w[e])

    h = make()
    drive(h, range(40))
    if path is not None:
        h["snap"].save(path)
        close(h)
        del h
        torch.cuda.empty_cache()
        h = make()
        assert h["snap"].load(path).tolist() == [13, -1, 0, 0]
    assert h["table"].begin_map(h["km"]).cpu().tolist() == [1, 40, 2, 0]
    drive(h, range(40, N))
    gate = api.ClosureGate(h["ctx"], h["src"], h["dst"], **sn.SCENE_GATE)
    work = torch.zeros((N, 12), dtype=torch.float64, device="cuda")
    a = h["table"].align_torch(h["src"], h["km"].poses, h["km"].state, out=work, optional=(), **c["align"])
    g = gate.run_torch(work, h["km"].state)
    out, rep = h["table"].relax_torch(h["dst"], work, h["km"].state, **sn.SCENE_RELAX)
    h["ctx"].sync()
    flat = lambda r: [x for x in (r if isinstance(r, (tuple, list)) else [r]) if torch.is_tensor(x)]
    res = dict(out=out.cpu().numpy(), rep=rep.cpu().numpy(), work=work.cpu().numpy())
    for name, r in (("align", a), ("gate", g)):
        for k, x in enumerate(flat(r)):
            res[f"{name}{k}"] = x.cpu().numpy()
    for part in ("km", "src", "dst", "table"):
        for nm in h[part].NAMES:
            res[f"{part}.{nm}"] = getattr(h[part], nm).cpu().numpy()
    gate.close()
    close(h)
    return res


def test_the_two_drive_scene_continues_to_the_same_bytes(tmp_path):
    c = sn.scene()
    want = two_drives(c, None)
    got = two_drives(c, str(tmp_path / "drive1.snap"))
    assert sorted(got) == sorted(want)
    for k in want:
        assert same_bytes(got[k], want[k]), k
    assert want["km.state"].tolist() == [80, 0, 0, 0] and want["src.state"][0] == 12 and want["table.state"][0] == 2 and want["dst.state"][0] == 9
    assert want["rep"][-1] == 78 + 9 and not same_bytes(want["out"], want["km.poses"])          # the chain did join the drives


# ------------------------------------------------------------------------------------------------ 6. continuation: the seq07 scene
@pytest.fixture(scope="module")
def seq07_clouds(golden_dir, tmp_path_factory):
    """the 110 keyframe clouds of the committed seq07 drive from the BATCH pre-stage (test_gpu_map.py's drive): no window state"""
    return seq07_batch_clouds(golden_dir, str(tmp_path_factory.mktemp("seq07s")))


S7_K, S7_MASK, S7_MAXC = 2, 5, 9000


def seq07_drive(cl, path):
    """generate -> match -> append -> map append -> align -> verify -> log, per keyframe.  path: keyframes 0 .. 54, SAVE, destroy every
    handle and free every buffer, create LARGER ones, LOAD, keyframes 55 .. 109; None: uninterrupted at the first capacities."""
    N = len(cl["ids"])
    sizes = np.diff(cl["offs"])
    assert sizes.max() <= S7_MAXC

    def make(kcap, pcap, ecap):
        ctx = _stream_context(0)
        km = api.KeyframeMap(ctx, kcap, pcap, S7_MAXC)
        odb = api.OnlineDatabase(ctx, "sc", kcap, max_k=S7_K)
        pgr = api.PoseGraph(ctx, kcap, ecap)
        return dict(ctx=ctx, km=km, odb=odb, pgr=pgr, snap=Snapshot(ctx, map=km, online=(odb,), graphs=(pgr,)))

    def close(h):
        for k in ("snap", "pgr", "odb", "km", "ctx"):
            h[k].close()

    x = torch.zeros((S7_MAXC, 3), dtype=torch.float64, device="cuda"); it = torch.zeros(S7_MAXC, dtype=torch.float32, device="cuda")
    offs = torch.zeros(2, dtype=torch.int64, device="cuda"); frame = torch.zeros(16, dtype=torch.float64, device="cuda")
    pose = torch.zeros((1, 12), dtype=torch.float64, device="cuda"); kid = torch.zeros(1, dtype=torch.int32, device="cuda")
    sig = torch.zeros((1, 2400), dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()
    res = []

    def step(h, k):
        a, b = int(cl["offs"][k]), int(cl["offs"][k + 1])
        x.zero_(); it.zero_()
        x[:b - a] = dev(cl["xyz"][a:b]); it[:b - a] = dev(cl["inten"][a:b], np.float32)
        offs.copy_(dev([0, b - a], np.int64)); frame.copy_(dev(cl["frames"][k])); pose.copy_(dev(cl["poses"][k][None])); kid.fill_(int(cl["ids"][k]))
        ctx, km, odb, pgr = h["ctx"], h["km"], h["odb"], h["pgr"]
        ctx.check(ctx.lib.pr_sc_generate_frames_dev(ctx.h, p(x), p(it), p(offs), 1, 45.0, p(frame), 1, p(sig)))
        idx, score, oinfo = odb.step_torch(sig, S7_MASK, 2.0, S7_K)
        minfo = km.append_torch(x, it, offs, frame, poses=pose, ids=kid)
        al = odb.align(idx, sig)
        T, stats, acc, hyp = km.verify_variants("sc", idx, al[0], (x, offs), frame[None], S7_MAXC, hypotheses=2, max_corr=1.0, min_fitness=0.5,
                                                max_rmse=0.5, max_iter=10)
        ginfo = pgr.add_torch(idx, T, acc, minfo[1:2])
        ctx.sync()
        res.append(dict(idx=idx.cpu().numpy(), score=score.cpu().numpy(), T=T.cpu().numpy(), stats=stats.cpu().numpy(), accepted=acc.cpu().numpy(),
                        oinfo=oinfo.cpu().numpy(), minfo=minfo.cpu().numpy(), ginfo=ginfo.cpu().numpy()))

    h = make(112, 1 << 18, 300)
    for k in range(55):
        step(h, k)
    if path is not None:
        h["snap"].save(path)
        close(h)
        del h
        torch.cuda.empty_cache()
        h = make(160, 1 << 19, 600)
        assert h["snap"].load(path).tolist() == [10, -1, 0, 0]
    for k in range(55, N):
        step(h, k)
    n = N
    pts = int(cl["offs"][N])
    E = int(h["pgr"].state.cpu()[0])
    state = {"km.state": h["km"].state, "odb.state": h["odb"].state, "pgr.state": h["pgr"].state, "xyz": h["km"].xyz[:pts], "inten": h["km"].inten[:pts],
             "offs": h["km"].offs[:n + 1], "frames": h["km"].frames[:n], "poses": h["km"].poses[:n], "ids": h["km"].ids[:n], "sig": h["odb"].sig[:n],
             "edge_ij": h["pgr"].edge_ij[:E], "edge_Z": h["pgr"].edge_Z[:E], "edge_w": h["pgr"].edge_w[:E]}
    state = {k: v.cpu().numpy() for k, v in state.items()}
    close(h)
    return res, state


def test_the_seq07_drive_continues_to_the_same_bytes(seq07_clouds, tmp_path):
    """Measured on an MI355X: the drive's sparse synthetic clouds give 3 accepted pairs of 220 and 3 logged edges;
    every keyframe's match, verify and log info is compared whether or not a pair was accepted."""
    want, wstate = seq07_drive(seq07_clouds, None)
    got, gstate = seq07_drive(seq07_clouds, str(tmp_path / "seq07.snap"))
    assert len(want) == len(got) == 110
    for k in range(110):                                  # from keyframe 55 on (and before it, where both runs are the same program)
        for name in ("idx", "score", "T", "stats", "accepted", "oinfo", "minfo", "ginfo"):
            assert same_bytes(got[k][name], want[k][name]), (k, name, got[k][name], want[k][name])
    for name in wstate:
        assert same_bytes(gstate[name], wstate[name]), name
    assert wstate["km.state"].tolist() == [110, 0, 0, 0] and wstate["odb.state"].tolist() == [110, 0, 0, 0]
    accepted = int(sum(r["accepted"].sum() for r in want))
    print("   accepted pairs over the drive:", accepted, "of", 110 * S7_K, "; edges logged:", int(wstate["pgr.state"][0]))
    assert int(wstate["pgr.state"][0]) == accepted and (want[109]["idx"] >= 0).all()
