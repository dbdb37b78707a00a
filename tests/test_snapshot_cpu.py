"""Snapshots (pr_snapshot) without a device: the rule text in the header, the ABI surface, the bound formula, the
argument errors and the host refusals of load that are returned before any device is touched, what the Python class refuses before it
calls the library, and properties of the NumPy restatement the GPU tests hold the kernels to (snapshot_np.py): pack then unpack is the
identity, and the checksum catches every single-bit flip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import snapshot_np as sp
from so_dso_place_recognition_amd import _lib, api, graph, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_snapshot_create", "pr_snapshot_destroy", "pr_snapshot_bound", "pr_snapshot_desc_bound", "pr_snapshot_pack_dev",
         "pr_snapshot_unpack_dev", "pr_snapshot_save", "pr_snapshot_load")
FLAGS = ("OVERFLOW", "BAD_MAGIC", "BAD_VERSION", "TRUNCATED", "MISSING", "CAPACITY", "CHECKSUM", "OFFSETS", "SESSIONS")


def test_snapshot_header_states_the_rule():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for words in ("pr_snapshot", "DESIGN.md 4.30", "OUT OF SCOPE", "fuse -> index -> normals", 'magic "PRASNAP1", version 1',
                  "pad64(b) = (b + 63) & ~63", "64 + 128 NS + sum over the sections of pad64(capacity rows x bytes per row)",
                  "x = w ^ ((i + 1) * 0x9E3779B97F4A7C15); x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27",
                  "x *= 0x94D049BB133111EB; x ^= x >> 31", "a 4-byte tail is", "a bijection of w", "64-bit integer atomic adds",
                  "No floating-point operation anywhere", "ONE", "No later", "3 launches (plan, copy, finish)",
                  "4 launches (header, sum, verify, scatter)", "info = {bytes written, sections, flags, 0}",
                  "nothing past the header's extent 64 + 128 NS is written", "would have been needed",
                  "clamped into its capacity before an address is formed from it", "points = offs[keyframes] in 0 .. point_capacity",
                  "the DESTINATION's capacity rows", "destination's max_cloud_points", "offs[0] != 0, descending at a row",
                  "start not strictly ascending", "Only extents that passed form an address", "switched off on the device by any failed check",
                  "left exactly as the destination held them", "info = {sections restored (NS or 0), first failing section or -1, flags, 0}",
                  "NO BYTE", 'path + ".tmp" and renamed', "exactly `bytes written`", "no device touched", "Two runs give the same bytes",
                  "xyz 24, inten 4: points | offs 8: keyframes + 1 | frames 128, poses 96, ids 4: keyframes"):
        assert words in txt, words
    for words in ("PRASNAP1", "0x9E3779B97F4A7C15", "zero-extended", "scatter only if every check passed"):
        assert words in sp.__doc__, words


def test_snapshot_symbols_records_and_class():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_snapshot_")) == sorted(NAMES)
    assert C.sizeof(_lib.SnapshotDesc) == 112 and _lib.SnapshotDesc.point_capacity.offset == 16 and _lib.SnapshotDesc.sessions.offset == 96
    for k, name in enumerate(FLAGS):
        assert re.search(r"PR_SNAPSHOT_%s = %d\b" % (name, 1 << k), code) and getattr(_lib, "SNAPSHOT_" + name) == 1 << k == getattr(sp, name)
    for k, name in enumerate(("MAP", "ONLINE", "ONLINESET", "GRAPH", "SESSION")):
        assert re.search(r"PR_SNAPSHOT_%s = %d\b" % (name, k + 1), code) and getattr(_lib, "SNAPSHOT_" + name) == k + 1 == getattr(sp, name)
    for m in ("bound", "pack_torch", "unpack_torch", "save", "load", "close"):
        assert hasattr(snapshot.Snapshot, m), m
    from so_dso_place_recognition_amd._handle import Handle
    assert issubclass(snapshot.Snapshot, Handle) and not hasattr(api, "Snapshot")               # not re-exported: api's names are pinned
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "snapshot.o: snapshot.hip snapshot.hpp" in mk and "snapshot_host.o: snapshot.cpp" in mk and " snapshot.o snapshot_host.o" in mk
    hip = open(os.path.join(CSRC, "snapshot.hip")).read()
    assert hip.count("atomicAdd(") == 1 and "atomicAdd(&sums[s], sh[0])" in hip                 # the one global atomic: a 64-bit integer add
    body = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"\b(double|float)\b", body)                                           # no floating-point operation


def _store():
    store = (C.c_double * 64)()
    return store, C.addressof(store)


def _desc(base, **kw):
    """a desc over host memory (never dereferenced: no device is touched) with every part, then edited by kw"""
    keep = []

    def rec(cls, n):
        r = cls(*([base + 16] * n)); keep.append(r)
        return C.addressof(r)
    d = _lib.SnapshotDesc()
    d.map, d.keyframe_capacity, d.point_capacity, d.max_cloud_points = rec(_lib.MapBuffers, 7), 8, 64, 16
    d.online[0], d.online_type[0], d.online_capacity[0] = rec(_lib.OnlineBuffers, 2), _lib.TYPE_SC, 8
    d.online[1], d.online_type[1], d.online_capacity[1] = rec(_lib.OnlineBuffers, 2), _lib.TYPE_M2DP, 8
    fs = _lib.OnlineSetBuffers(base, base, None, base); keep.append(fs)
    d.onlineset, d.onlineset_kind, d.onlineset_capacity = C.addressof(fs), _lib.ONLINESET_FUSED, 8
    d.graph[0], d.edge_capacity[0] = rec(_lib.PoseGraphBuffers, 4), 4
    d.graph[1], d.edge_capacity[1] = rec(_lib.PoseGraphBuffers, 4), 4
    d.sessions, d.session_capacity = rec(_lib.SessionBuffers, 2), 2
    for k, val in kw.items():
        if isinstance(val, tuple):
            getattr(d, k)[val[0]] = val[1]
        else:
            setattr(d, k, val)
    d._keep = keep
    return d


def _np_state(kc=None, pc=None, mcp=None, on=(), fused=None, delight=None, ec=(), sc=None):
    st = []
    if kc:
        st.append(sp.map_part(kc, pc, mcp))
    st += [sp.online_part(t, c) for t, c in on]
    if fused:
        st.append(sp.set_part(sp.SET_FUSED, fused))
    if delight:
        st.append(sp.set_part(sp.SET_DELIGHT, delight))
    st += [sp.graph_part(k, c) for k, c in enumerate(ec)]
    if sc:
        st.append(sp.session_part(sc))
    return st


def test_snapshot_bound_formula():
    lib = _lib.load()
    _, base = _store()
    b = C.c_int64()
    cases = ((8, 64, 16, 8, 8, 8, 4, 4, 2), (1, 1, 1, 1, 1, 1, 1, 1, 1), (3475, 3475 * 400, 400, 3475, 3475, 40, 173, 173, 8),
             (110, 110 * 2048, 2048, 110, 110, 110, 600, 600, 4), (65, 513, 257, 3, 5, 7, 513, 1, 1024))
    for kc, pc, mcp, c0, c1, cs, e0, e1, sc in cases:
        d = _desc(base, keyframe_capacity=kc, point_capacity=pc, max_cloud_points=mcp, online_capacity=(0, c0), onlineset_capacity=cs,
                  session_capacity=sc)
        d.online_capacity[1], d.edge_capacity[0], d.edge_capacity[1] = c1, e0, e1
        assert lib.pr_snapshot_desc_bound(C.byref(d), C.byref(b)) == 0, lib.pr_last_error(None)
        st = _np_state(kc, pc, mcp, ((sp.TYPE_SC, c0), (sp.TYPE_M2DP, c1)), fused=cs, ec=(e0, e1), sc=sc)
        by_hand = 64 + 128 * 17 + sum(sp.pad64(x) for x in (24 * pc, 4 * pc, 8 * (kc + 1), 128 * kc, 96 * kc, 4 * kc, 19200 * c0, 12288 * c1,
                                                           19200 * cs, 12288 * cs, 8 * e0, 96 * e0, 16 * e0, 8 * e1, 96 * e1, 16 * e1, 4 * sc))
        assert b.value == sp.bound(st) == by_hand, (kc, pc)
    d = _desc(base, map=None, onlineset_kind=_lib.ONLINESET_DELIGHT)                 # parts alone: a DELIGHT set, one log
    d.online[0] = d.online[1] = d.graph[1] = d.sessions = None
    ds = _lib.OnlineSetBuffers(None, None, base, base)
    d.onlineset = C.addressof(ds)
    assert lib.pr_snapshot_desc_bound(C.byref(d), C.byref(b)) == 0, lib.pr_last_error(None)
    assert b.value == sp.bound(_np_state(delight=8, ec=(4,))) == 64 + 128 * 4 + 8 * 32768 + 64 + 384 + 64


def test_snapshot_argument_errors_before_any_device():
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    store, base = _store()

    def create(d=True, out=True):
        h = C.c_void_p(1)
        rc = lib.pr_snapshot_create(None, C.byref(d) if d is not None else None, C.byref(h) if out else None)
        assert rc == _lib.PR_EINVAL and (not out or not h.value)
        return err()

    assert "out is NULL" in create(_desc(base), out=False) and "desc is NULL" in create(None)
    empty = _lib.SnapshotDesc()
    assert "names no part" in create(empty)
    assert "ctx is NULL" in create(_desc(base))                                      # the last check: everything else was in order
    for field, text in (("keyframe_capacity", "keyframe_capacity=%d outside"), ("point_capacity", "point_capacity=%d outside"),
                        ("max_cloud_points", "max_cloud_points=%d outside"), ("onlineset_capacity", "onlineset_capacity=%d outside"),
                        ("session_capacity", "session_capacity=%d outside")):
        for bad in (0, -1):
            assert text % bad in create(_desc(base, **{field: bad})), field
    assert "max_cloud_points=65 outside 1 .. point_capacity=64" in create(_desc(base, max_cloud_points=65))
    assert "session_capacity=1025" in create(_desc(base, session_capacity=1025))
    for k in (0, 1):
        for bad in (0, -1):
            assert "online_capacity[%d]=%d outside" % (k, bad) in create(_desc(base, online_capacity=(k, bad)))
            assert "edge_capacity[%d]=%d outside" % (k, bad) in create(_desc(base, edge_capacity=(k, bad)))
        for bad in (-1, 2, _lib.TYPE_DELIGHT + 5):
            assert "online_type[%d]=%d is neither" % (k, bad) in create(_desc(base, online_type=(k, bad)))
    for bad in (-1, 2):
        assert "onlineset_kind=%d is neither" % bad in create(_desc(base, onlineset_kind=bad))
    assert "do not fit its kind" in create(_desc(base, onlineset_kind=_lib.ONLINESET_DELIGHT))          # fused buffers under the DELIGHT kind
    for name in api.KeyframeMap.NAMES:
        d = _desc(base); r = _lib.MapBuffers(*([base] * 7)); setattr(r, name, None); d.map = C.addressof(r)
        assert "a buffer of the map is NULL" in create(d), name
    for name in api.PoseGraph.NAMES:
        d = _desc(base); r = _lib.PoseGraphBuffers(*([base] * 4)); setattr(r, name, None); d.graph[1] = C.addressof(r)
        assert "a buffer of closure log 1 is NULL" in create(d), name
    for name in graph.SessionTable.NAMES:
        d = _desc(base); r = _lib.SessionBuffers(base, base); setattr(r, name, None); d.sessions = C.addressof(r)
        assert "a buffer of the session table is NULL" in create(d), name
    b = C.c_int64(7)
    assert lib.pr_snapshot_bound(None, C.byref(b)) == _lib.PR_EINVAL and "pr_snapshot_bound: snapshot is NULL" in err()
    assert lib.pr_snapshot_bound(None, None) == _lib.PR_EINVAL and "bytes is NULL" in err()
    assert lib.pr_snapshot_desc_bound(None, C.byref(b)) == _lib.PR_EINVAL and "desc is NULL" in err() and b.value == 0
    assert lib.pr_snapshot_desc_bound(C.byref(empty), C.byref(b)) == _lib.PR_EINVAL and "names no part" in err()
    lib.pr_snapshot_destroy(None)                        # a no-op
    blob = (base + 15) & ~15
    for fn in ("pr_snapshot_pack_dev", "pr_snapshot_unpack_dev"):
        f = getattr(lib, fn)
        assert f(None, None, 64, base) == _lib.PR_EINVAL and fn + ": the blob is NULL" in err()
        assert f(None, blob, 64, None) == _lib.PR_EINVAL and fn + ": info is NULL" in err()
        assert f(None, blob, -1, base) == _lib.PR_EINVAL and "negative blob size" in err()
        assert f(None, blob + 8, 64, base) == _lib.PR_EINVAL and "16-byte boundary" in err()
        assert f(None, blob, 64, base) == _lib.PR_EINVAL and fn + ": snapshot is NULL" in err()
    assert lib.pr_snapshot_save(None, None) == _lib.PR_EINVAL and "pr_snapshot_save: path is NULL" in err()
    assert lib.pr_snapshot_save(None, b"") == _lib.PR_EINVAL and "path is NULL or empty" in err()
    assert lib.pr_snapshot_save(None, b"/nonexistent/x") == _lib.PR_EINVAL and "pr_snapshot_save: snapshot is NULL" in err()
    assert lib.pr_snapshot_load(None, None, base) == _lib.PR_EINVAL and "pr_snapshot_load: path is NULL" in err()
    assert lib.pr_snapshot_load(None, b"x", None) == _lib.PR_EINVAL and "pr_snapshot_load: info is NULL" in err()


def test_snapshot_load_refuses_on_the_host(tmp_path):
    """every refusal returns with a NULL handle still unexamined: the file checks come first and touch no device"""
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    info = (C.c_int64 * 4)()
    load = lambda p: lib.pr_snapshot_load(None, os.fsencode(str(p)), info)
    assert load(tmp_path / "missing.snap") == _lib.PR_EIO and "cannot open" in err()
    st = _np_state(8, 64, 16, ((sp.TYPE_M2DP, 4),), ec=(4,), sc=2)
    sp.fill(st[0], 1, 5); sp.fill(st[1], 2, 3); sp.fill(st[2], 3, 2); sp.fill(st[3], 4, 2)
    blob, binfo = sp.pack(st)
    ext = 64 + 128 * 11
    for name, raw, text in (("empty", b"", "shorter than a header"), ("short", blob[:63].tobytes(), "shorter than a header"),
                            ("cut", blob[:ext - 1].tobytes(), "cut inside its header"), ("cut2", blob[:64].tobytes(), "cut inside its header"),
                            ("past", blob[:binfo[0] - 64].tobytes(), "points outside the file")):
        p = tmp_path / name
        p.write_bytes(raw)
        assert load(p) == _lib.PR_EINVAL and text in err(), name
    bad = blob.copy()
    bad[64 + 128 * 3 + 40:64 + 128 * 3 + 48] = np.array([-64], np.int64).view(np.uint8)       # a negative offset in the table
    (tmp_path / "neg").write_bytes(bad.tobytes())
    assert load(tmp_path / "neg") == _lib.PR_EINVAL and "section 3" in err() and "points outside the file" in err()
    (tmp_path / "whole").write_bytes(blob.tobytes())                                 # a file in order reaches the handle check, the last one
    assert load(tmp_path / "whole") == _lib.PR_EINVAL and "pr_snapshot_load: snapshot is NULL" in err()


def test_snapshot_class_refuses_before_the_library():
    import torch

    class Fake:
        pass
    ctx = Fake(); ctx.lib = None
    km, pgf = Fake(), Fake()
    km.ctx, pgf.ctx = ctx, object()
    with pytest.raises(ValueError, match="share one context"):
        snapshot.Snapshot(ctx, map=km, graphs=(pgf,))
    with pytest.raises(ValueError, match="no part was given"):
        snapshot.Snapshot(ctx)
    with pytest.raises(ValueError, match="at most two"):
        snapshot.Snapshot(ctx, online=(km, km, km))
    with pytest.raises(ValueError, match="at most two"):
        snapshot.Snapshot(ctx, graphs=(km, km, km))
    s = snapshot.Snapshot.__new__(snapshot.Snapshot)     # no handle, no library call: the checks are the first thing a method does
    s.ctx, s.h = ctx, None
    cpu = torch.zeros(64, dtype=torch.uint8)
    for call in (lambda: s.pack_torch(cpu), lambda: s.unpack_torch(cpu, 64)):
        with pytest.raises(ValueError, match="blob must be a contiguous CUDA tensor"):
            call()
    s.close()                                            # never created: no library call


# ------------------------------------------------------------------------------------------------ the restatement
def _random_state(seed):
    r = np.random.default_rng(seed)
    kc, mcp = int(r.integers(1, 40)), int(r.integers(1, 70))
    pc = kc * mcp + int(r.integers(0, 9))
    st = _np_state(kc, pc, mcp, ((sp.TYPE_SC, int(r.integers(1, 5))), (sp.TYPE_M2DP, int(r.integers(1, 6)))), fused=int(r.integers(1, 4)),
                   ec=(int(r.integers(1, 30)), int(r.integers(1, 9))), sc=int(r.integers(1, 9)))
    for k, p in enumerate(st):
        sp.fill(p, seed * 16 + k, int(r.integers(0, p["caps"][0] + 1)))
    return st


@pytest.mark.parametrize("seed", range(6))
def test_pack_then_unpack_is_the_identity(seed):
    st = _random_state(seed)
    blob, info = sp.pack(st)
    assert info.tolist() == [blob.size, 17, 0, 0] and blob.size % 64 == 0 and blob.size <= sp.bound(st)
    d = sp.describe(blob)
    assert d["total"] == blob.size and all(e["offset"] % 64 == 0 for e in d["table"])
    # into equal capacities and into larger ones; the rows at and above the counts keep the destination's bytes
    for grow in (0, 1):
        kc, pc, mcp = (c * (1 + grow) + grow for c in st[0]["caps"][:3])
        dst = _np_state(kc, pc, mcp, tuple((p["subtype"], p["caps"][0] + grow) for p in st[1:3]), fused=st[3]["caps"][0] + grow,
                        ec=tuple(p["caps"][0] * (1 + grow) for p in st[4:6]), sc=st[6]["caps"][0] + grow)
        for p in dst:
            for a in p["arrays"].values():
                a.reshape(-1).view(np.uint8)[:] = 0x5C
        before = sp.copy_state(dst)
        info = sp.unpack(dst, blob)
        assert info.tolist() == [17, -1, 0, 0]
        for p, q, b in zip(st, dst, before):
            assert q["state"].tobytes() == p["state"].tobytes()
            n, pts = sp.counts(p)
            for name, bpr, which in p["sections"]:
                rows = pts if which == "pts" else (n + 1 if which == "n1" else n)
                got, src, old = (x["arrays"][name].reshape(-1).view(np.uint8) for x in (q, p, b))
                assert got[:rows * bpr].tobytes() == src[:rows * bpr].tobytes() and got[rows * bpr:].tobytes() == old[rows * bpr:].tobytes(), name
        again, _ = sp.pack(dst)
        assert again[64 + 128 * 17:].tobytes() == blob[64 + 128 * 17:].tobytes()                  # the sections; the table records other capacities
        if not grow:
            assert again.tobytes() == blob.tobytes()


def test_every_single_bit_flip_in_a_section_is_caught():
    st = _random_state(11)
    blob, _ = sp.pack(st)
    d = sp.describe(blob)
    live = [e for e in d["table"] if e["length"]]
    r = np.random.default_rng(2024)
    clean = sp.copy_state(st)
    for trial in range(1000):
        e = live[int(r.integers(len(live)))]
        byte, bit = e["offset"] + int(r.integers(e["length"])), int(r.integers(8))
        bad = blob.copy()
        bad[byte] ^= 1 << bit
        assert sp.checksum(bad[e["offset"]:e["offset"] + e["length"]]) != e["checksum"] % (1 << 64), (trial, byte, bit)
        if trial < 40:                                   # and the validator names it and leaves the destination alone
            info, _ = sp.validate(st, bad)
            assert info[2] & sp.CHECKSUM and info[0] == 0 and info[1] <= d["table"].index(e)
            assert sp.unpack(st, bad)[0] == 0 and sp.state_bytes(st) == sp.state_bytes(clean)
    # the tail rule: a 4-byte tail is zero-extended, and the word index matters (a permutation of words changes the sum)
    w = np.arange(5, dtype=np.uint32)
    assert sp.checksum(w.tobytes()) == sp.checksum(np.append(w, np.uint32(0)).tobytes()) != sp.checksum(w[::-1].copy().tobytes())
    assert sp.checksum(b"") == 0 and sp.mix(0, 0) != 0


def test_the_validator_names_each_failure():
    st = _np_state(8, 64, 16, ((sp.TYPE_M2DP, 4),), ec=(4,), sc=4)
    sp.fill(st[0], 1, 5, cloud_sizes=[3, 0, 16, 1, 7]); sp.fill(st[1], 2, 3); sp.fill(st[2], 3, 2); sp.fill(st[3], 4, 3)
    blob, _ = sp.pack(st)
    ok = lambda b, n=None, dst=st: sp.validate(dst, b, n)[0].tolist()
    assert ok(blob) == [11, -1, 0, 0]
    b = blob.copy(); b[0] ^= 1
    assert ok(b) == [0, -1, sp.BAD_MAGIC, 0]
    b = blob.copy(); b[8] += 1
    assert ok(b) == [0, -1, sp.BAD_VERSION, 0]
    assert ok(blob, 63) == [0, -1, sp.TRUNCATED, 0] and ok(blob, blob.size - 64)[1:3] == [10, sp.TRUNCATED]
    d = sp.describe(blob)
    o = d["table"][2]["offset"]                                                       # the map's offs
    b = blob.copy(); b[o:o + 8] = np.array([1], np.int64).view(np.uint8)
    assert ok(b)[1:3] == [2, sp.CHECKSUM | sp.OFFSETS]
    small = _np_state(8, 64, 15, ((sp.TYPE_M2DP, 4),), ec=(4,), sc=4)                 # a cloud of 16 above max_cloud_points = 15
    assert ok(blob, dst=small) == [0, 2, sp.CAPACITY, 0]
    for dst, s in ((_np_state(4, 64, 16, ((sp.TYPE_M2DP, 4),), ec=(4,), sc=4), 2), (_np_state(8, 26, 16, ((sp.TYPE_M2DP, 4),), ec=(4,), sc=4), 0),
                   (_np_state(8, 64, 16, ((sp.TYPE_M2DP, 2),), ec=(4,), sc=4), 6), (_np_state(8, 64, 16, ((sp.TYPE_M2DP, 4),), ec=(1,), sc=4), 7),
                   (_np_state(8, 64, 16, ((sp.TYPE_M2DP, 4),), ec=(4,), sc=2), 10)):
        assert ok(blob, dst=dst) == [0, s, sp.CAPACITY, 0], s
    assert ok(blob, dst=_np_state(8, 64, 16, ((sp.TYPE_SC, 4),), ec=(4,), sc=4)) == [0, 6, sp.MISSING, 0]
    assert ok(blob, dst=_np_state(8, 64, 16, ec=(4,), sc=4))[1:3] == [6, sp.MISSING]
    b = blob.copy(); b[64 + 128 * 7 + 24] ^= 1                                        # a flipped count in the table
    assert ok(b)[1:3] == [7, sp.CHECKSUM | sp.TRUNCATED] and ok(sp.retable(b))[1:3] == [7, sp.TRUNCATED]
    so = d["table"][10]["offset"]
    b = blob.copy(); b[so + 4:so + 8] = 0
    assert ok(b)[1:3] == [10, sp.CHECKSUM | sp.SESSIONS]
    # a blob that would not fit: the header alone, the needed size, zero checksums
    full, info = sp.pack(st)
    head, hinfo = sp.pack(st, blob_capacity=full.size - 1)
    assert hinfo.tolist() == [full.size, 11, sp.OVERFLOW, 0] and head.size == 64 + 128 * 11 and all(e["checksum"] == 0 for e in sp.describe(head)["table"])
    none, ninfo = sp.pack(st, blob_capacity=64 + 128 * 11 - 1)
    assert none.size == 0 and ninfo.tolist() == hinfo.tolist()
    # scribbled counts are clamped, the state words travel verbatim
    sc = sp.copy_state(st)
    sc[0]["state"][0] = 1 << 30; sc[0]["arrays"]["offs"][8] = 1 << 40; sc[1]["state"][0] = -7
    d2 = sp.describe(sp.pack(sc)[0])
    assert [e["rows"] for e in d2["table"][:7]] == [64, 64, 9, 8, 8, 8, 0] and d2["table"][0]["state"][0] == 1 << 30 and d2["table"][6]["state"][0] == -7
