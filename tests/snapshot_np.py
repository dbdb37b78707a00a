"""NumPy restatement of the snapshot format (pr_snapshot; the rule text is in include/place_recognition.h): a writer, a
reader and a validator of the blob.  It is what the device is held to byte for byte, and it makes or inspects a file without a device.

A STATE is a list of parts in blob order (map, online[0], online[1], online set, graph[0], graph[1], sessions); a part is a dict
  kind, subtype, caps (4 ints: the count's capacity first), count_min, state (int32 [4]), arrays {name: ndarray at full capacity}
made by map_part / online_part / set_part / graph_part / session_part.  The arrays are the caller-owned buffers of the C records.

  blob      header 8 x i64 (magic "PRASNAP1", version 1, NS, total bytes, 64 + 128 NS, table checksum, 0, 0) | table NS x 16 x i64 (kind,
            subtype, array, rows, bytes per row, offset, length, checksum, state words 2 x i64, capacities 4 x i64, part, 0) | the live
            rows of every section, each section on a 64-byte boundary, zero pad behind it
  checksum  wrap-around uint64 sum over the 8-byte words w_i of mix(w_i, i), a 4-byte tail zero-extended;
            mix: x = w ^ ((i + 1) * 0x9E3779B97F4A7C15); x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
  pack      counts clamped into their capacities, the map's offs[keyframes] into 0 .. point_capacity; info = bytes, sections, flags, 0;
            a blob that would not fit: OVERFLOW, header and table with zero checksums only, bytes = the size needed
  unpack    validate (flags and the first failing section as the header states them), then scatter only if every check passed
"""
import numpy as np

MAGIC, VERSION = 0x3150414E53415250, 1
HEADER, ENTRY, MAX_SECTIONS = 64, 128, 17
MAP, ONLINE, ONLINESET, GRAPH, SESSION = 1, 2, 3, 4, 5
OVERFLOW, BAD_MAGIC, BAD_VERSION, TRUNCATED, MISSING, CAPACITY, CHECKSUM, OFFSETS, SESSIONS = 1, 2, 4, 8, 16, 32, 64, 128, 256
TYPE_SC, TYPE_M2DP, SET_FUSED, SET_DELIGHT = 0, 1, 0, 1
SIG_ROWS = {TYPE_SC: (1, 2400), TYPE_M2DP: (4, 384)}                   # rows per entry, row length
# (array, bytes per row, which count) of every kind; "pts": the map's points, "n1": count + 1, "n": count
MAP_SECTIONS = (("xyz", 24, "pts"), ("inten", 4, "pts"), ("offs", 8, "n1"), ("frames", 128, "n"), ("poses", 96, "n"), ("ids", 4, "n"))
GRAPH_SECTIONS = (("edge_ij", 8, "n"), ("edge_Z", 96, "n"), ("edge_w", 16, "n"))
_U = np.uint64


def pad64(b):
    return (int(b) + 63) & ~63


def mix(w, i):
    """the fixed integer mix of (word, word index) on uint64 arrays (wrap-around)"""
    w, i = np.asarray(w, _U), np.asarray(i, _U)
    with np.errstate(over="ignore"):
        x = w ^ ((i + _U(1)) * _U(0x9E3779B97F4A7C15))
        x = x ^ (x >> _U(30)); x = x * _U(0xBF58476D1CE4E5B9)
        x = x ^ (x >> _U(27)); x = x * _U(0x94D049BB133111EB)
        x = x ^ (x >> _U(31))
    return x


def checksum(raw) -> int:
    """of a section's bytes (a multiple of 4): the sum of mix over its 8-byte words, a 4-byte tail zero-extended"""
    b = np.frombuffer(bytes(raw), np.uint8)
    if b.size % 8:
        b = np.concatenate([b, np.zeros(8 - b.size % 8, np.uint8)])
    w = b.view("<u8")
    with np.errstate(over="ignore"):
        return int(mix(w, np.arange(w.size, dtype=_U)).sum(dtype=_U))


# ------------------------------------------------------------------------------------------------ parts
def _part(kind, subtype, caps, count_min, sections, arrays, state):
    caps = [int(c) for c in caps] + [0] * (4 - len(caps))
    return dict(kind=kind, subtype=subtype, caps=caps, count_min=count_min, sections=tuple(sections), arrays=arrays,
                state=np.zeros(4, np.int32) if state is None else state)


def map_part(kc, pc, mcp, arrays=None, state=None):
    a = arrays or dict(xyz=np.zeros((pc, 3)), inten=np.zeros(pc, np.float32), offs=np.zeros(kc + 1, np.int64), frames=np.zeros((kc, 16)),
                       poses=np.zeros((kc, 12)), ids=np.zeros(kc, np.int32))
    return _part(MAP, 0, (kc, pc, mcp), 0, MAP_SECTIONS, a, state)


def online_part(type_, cap, arrays=None, state=None):
    r, L = SIG_ROWS[type_]
    return _part(ONLINE, type_, (cap,), 0, (("sig", 8 * r * L, "n"),), arrays or dict(sig=np.zeros((cap * r, L))), state)


def set_part(kind, cap, arrays=None, state=None):
    if kind == SET_FUSED:
        return _part(ONLINESET, kind, (cap,), 0, (("sc", 19200, "n"), ("m2dp", 12288, "n")),
                     arrays or dict(sc=np.zeros((cap, 2400)), m2dp=np.zeros((cap * 4, 384))), state)
    return _part(ONLINESET, kind, (cap,), 0, (("delight", 32768, "n"),), arrays or dict(delight=np.zeros((cap * 16, 256))), state)


def graph_part(slot, ec, arrays=None, state=None):
    a = arrays or dict(edge_ij=np.zeros((ec, 2), np.int32), edge_Z=np.zeros((ec, 12)), edge_w=np.zeros((ec, 2)))
    return _part(GRAPH, slot, (ec,), 0, GRAPH_SECTIONS, a, state)


def session_part(sc, arrays=None, state=None):
    st = np.array([1, 0, 0, 0], np.int32) if state is None else state
    return _part(SESSION, 0, (sc,), 1, (("start", 4, "n"),), arrays or dict(start=np.zeros(sc, np.int32)), st)


def cap_rows(part, which):
    c = part["caps"]
    return c[1] if which == "pts" else (c[0] + 1 if which == "n1" else c[0])


def sections(state):
    """[(part index, part, array index, name, bytes per row, which count)] in blob order"""
    return [(p, part, a, name, bpr, which) for p, part in enumerate(state) for a, (name, bpr, which) in enumerate(part["sections"])]


def bound(state) -> int:
    """the largest blob the capacities can produce: the header's formula"""
    secs = sections(state)
    return HEADER + ENTRY * len(secs) + sum(pad64(cap_rows(part, which) * bpr) for _, part, _, _, bpr, which in secs)


def counts(part):
    """(count, points) clamped as the pack clamps them"""
    c = part["caps"]
    n = min(max(int(part["state"][0]), part["count_min"]), c[0])
    pts = min(max(int(part["arrays"]["offs"][n]), 0), c[1]) if part["kind"] == MAP else 0
    return n, pts


# ------------------------------------------------------------------------------------------------ the writer
def pack(state, blob_capacity=None):
    """-> (blob uint8 [bytes written to the blob], info int64 [4]).  With blob_capacity too small: OVERFLOW, the header and table alone
    (nothing at all when even they do not fit) and info[0] = the size that would have been needed."""
    secs = sections(state)
    ns = len(secs)
    ext = HEADER + ENTRY * ns
    off, rows_of, raws = ext, [], []
    for p, part, a, name, bpr, which in secs:
        n, pts = counts(part)
        rows = pts if which == "pts" else (n + 1 if which == "n1" else n)
        raw = np.ascontiguousarray(part["arrays"][name]).reshape(-1).view(np.uint8)[:rows * bpr]
        rows_of.append((rows, off, rows * bpr))
        raws.append(raw)
        off += pad64(rows * bpr)
    total = off
    fits = blob_capacity is None or total <= blob_capacity
    table = np.zeros((ns, 16), np.int64)
    for s, ((p, part, a, name, bpr, which), (rows, o, ln)) in enumerate(zip(secs, rows_of)):
        cs = np.array([checksum(raws[s]) if fits else 0], _U).view(np.int64)[0]
        table[s, :8] = (part["kind"], part["subtype"], a, rows, bpr, o, ln, cs)
        table[s, 8:10] = np.asarray(part["state"], np.int32).view(np.int64)
        table[s, 10:14] = part["caps"]
        table[s, 14] = p
    tsum = np.array([checksum(table.tobytes())], _U).view(np.int64)[0]
    header = np.array([MAGIC, VERSION, ns, total, ext, tsum, 0, 0], np.int64)
    info = np.array([total, ns, 0 if fits else OVERFLOW, 0], np.int64)
    if not fits:
        head = np.concatenate([header.view(np.uint8), table.reshape(-1).view(np.uint8)])
        return (head if ext <= blob_capacity else np.zeros(0, np.uint8)), info
    blob = np.zeros(total, np.uint8)
    blob[:HEADER] = header.view(np.uint8)
    blob[HEADER:ext] = table.reshape(-1).view(np.uint8)
    for raw, (rows, o, ln) in zip(raws, rows_of):
        blob[o:o + ln] = raw
    return blob, info


def retable(blob):
    """recomputes the table's checksum of a blob whose table was edited on purpose (in place)"""
    ns = int(blob[16:24].view(np.int64)[0])
    blob[40:48] = np.array([checksum(blob[HEADER:HEADER + ENTRY * ns])], _U).view(np.uint8)
    return blob


# ------------------------------------------------------------------------------------------------ the reader and validator
def validate(state, blob, nbytes=None):
    """the checks of pr_snapshot_unpack_dev against the DESTINATION state -> (info int64 [4], plan); plan[s] = (rows, offset, length) of
    the sections that passed the table checks, None for the others"""
    blob = np.ascontiguousarray(blob, np.uint8)
    nbytes = blob.size if nbytes is None else int(nbytes)
    secs = sections(state)
    ns = len(secs)
    flags, first = 0, [1 << 31]
    plan = [None] * ns

    def fail(s):
        first[0] = min(first[0], s)

    def done():
        ok = flags == 0
        return np.array([ns if ok else 0, -1 if first[0] == 1 << 31 else first[0], flags, 0], np.int64), plan

    if nbytes < HEADER:
        flags |= TRUNCATED
        return done()
    h = blob[:HEADER].view(np.int64)
    if h[0] != MAGIC:
        flags |= BAD_MAGIC
        return done()
    if h[1] != VERSION:
        flags |= BAD_VERSION
        return done()
    nsec = int(h[2])
    if nsec < 0 or nsec > MAX_SECTIONS or HEADER + ENTRY * nsec > nbytes:
        flags |= TRUNCATED
        return done()
    table = blob[HEADER:HEADER + ENTRY * nsec].view(np.int64).reshape(nsec, 16)
    if np.array([checksum(table.tobytes())], _U).view(np.int64)[0] != h[5]:
        flags |= CHECKSUM                                   # the table's own checksum names no section
    if nsec != ns:
        flags |= MISSING
        fail(min(nsec, ns))
    prev_end = HEADER + ENTRY * nsec
    for s in range(min(ns, nsec)):
        p, part, a, name, bpr, which = secs[s]
        e = [int(x) for x in table[s]]
        rows, off, ln = e[3], e[5], e[6]
        bad = 0
        if (e[0], e[1], e[2], e[4]) != (part["kind"], part["subtype"], a, bpr):
            bad = MISSING
        elif rows < 0 or rows > cap_rows(part, which):
            bad = CAPACITY
        elif ln != rows * bpr or off < prev_end or off % 64 or off > nbytes or ln > nbytes - off:
            bad = TRUNCATED
        if bad:
            flags |= bad
            fail(s)
            continue
        plan[s] = (rows, off, ln)
        prev_end = off + pad64(ln)
    for p, part in enumerate(state):                        # the sections of one part agree on its counts
        want = {}
        for s, (q, _, a, name, bpr, which) in enumerate(secs):
            if q != p or plan[s] is None:
                continue
            key = "pts" if which == "pts" else "n"
            r = plan[s][0] - 1 if which == "n1" else plan[s][0]
            if key not in want and r >= 0:
                want[key] = r
            elif r != want.get(key, -1):
                flags |= TRUNCATED
                fail(s)
    for s, (p, part, a, name, bpr, which) in enumerate(secs):
        if plan[s] is None:
            continue
        rows, off, ln = plan[s]
        if np.array([checksum(blob[off:off + ln])], _U).view(np.int64)[0] != table[s, 7]:
            flags |= CHECKSUM
            fail(s)
        if part["kind"] == MAP and which == "n1":
            o = blob[off:off + ln].view(np.int64)
            n, bad = rows - 1, 0
            if n < 0:
                bad |= OFFSETS
            else:
                d = np.diff(o)
                if (d < 0).any():
                    bad |= OFFSETS
                if ((d >= 0) & (d > part["caps"][2])).any():
                    bad |= CAPACITY
                if o[0] != 0:
                    bad |= OFFSETS
                sx = next(t for t, q in enumerate(secs) if q[0] == p)        # the part's first section holds the points
                if plan[sx] is not None and o[n] != plan[sx][0]:
                    bad |= OFFSETS
            if bad:
                flags |= bad
                fail(s)
        if part["kind"] == SESSION:
            st = blob[off:off + ln].view(np.int32)
            if rows < 1 or st[0] != 0 or (np.diff(st.astype(np.int64)) <= 0).any():
                flags |= SESSIONS
                fail(s)
    return done()


def unpack(state, blob, nbytes=None):
    """validates; if every check passed, copies the saved rows and state words into the destination state IN PLACE -> info"""
    blob = np.ascontiguousarray(blob, np.uint8)
    info, plan = validate(state, blob, nbytes)
    if info[2] != 0:
        return info
    for s, (p, part, a, name, bpr, which) in enumerate(sections(state)):
        rows, off, ln = plan[s]
        part["arrays"][name].reshape(-1).view(np.uint8)[:ln] = blob[off:off + ln]
        if a == 0:
            part["state"][:] = blob[HEADER + ENTRY * s + 64:HEADER + ENTRY * s + 80].view(np.int32)
    return info


def describe(blob):
    """the header and table of a blob as Python values (no validation beyond what reading them needs)"""
    blob = np.ascontiguousarray(blob, np.uint8)
    h = blob[:HEADER].view(np.int64)
    ns = int(h[2])
    t = blob[HEADER:HEADER + ENTRY * ns].view(np.int64).reshape(ns, 16)
    keys = ("kind", "subtype", "array", "rows", "row_bytes", "offset", "length", "checksum")
    return dict(magic=int(h[0]), version=int(h[1]), sections=ns, total=int(h[3]), extent=int(h[4]),
                table=[dict(zip(keys, (int(x) for x in r[:8])), state=r[8:10].view(np.int32).tolist(), caps=r[10:14].tolist(), part=int(r[14]))
                       for r in t])


# ------------------------------------------------------------------------------------------------ states for the tests
def fill(part, seed, n, cloud_sizes=None):
    """random live rows below the count n (for a map: clouds of the given sizes, which must fit), a fill pattern above"""
    r = np.random.default_rng(seed)
    for name, arr in part["arrays"].items():
        flat = arr.reshape(-1).view(np.uint8)
        flat[:] = 0xA5                                                          # the fill pattern of rows at and above the count
    a = part["arrays"]
    if part["kind"] == MAP:
        sizes = np.asarray(cloud_sizes if cloud_sizes is not None else r.integers(0, part["caps"][2] + 1, n), np.int64)[:n]
        a["offs"][:] = 0
        a["offs"][1:n + 1] = np.cumsum(sizes)
        pts = int(a["offs"][n])
        assert pts <= part["caps"][1] and (sizes <= part["caps"][2]).all()
        a["xyz"][:pts] = r.standard_normal((pts, 3)) * 30.0
        a["inten"][:pts] = r.random(pts, np.float32)
        a["frames"][:n] = r.standard_normal((n, 16))
        a["frames"][:n][sizes == 0] = 0.0                                       # an empty or dropped row has a zero frame
        a["poses"][:n] = r.standard_normal((n, 12))
        a["ids"][:n] = r.integers(-1, 1 << 20, n)
        a["frames"][n:] = 0.0                                                   # (the map's own invariant for rows >= keyframes)
    elif part["kind"] == SESSION:
        n = max(n, 1)
        a["start"][:n] = np.concatenate([[0], np.cumsum(r.integers(1, 9, n - 1))])
    else:
        for name, bpr, _ in part["sections"]:
            arr = a[name]
            rows = n * (arr.shape[0] // max(part["caps"][0], 1))
            if arr.dtype == np.int32:
                arr[:rows] = r.integers(0, 1 << 20, arr[:rows].shape)
            else:
                arr[:rows] = r.standard_normal(arr[:rows].shape)
                if rows:
                    arr[0, 0] = np.nan                                          # raw IEEE bytes: a NaN and a -0.0 survive bit for bit
                    arr[rows - 1, -1] = -0.0
    part["state"][:] = (n, int(r.integers(0, 2)), 0, 0)                         # a sticky flag travels with the count
    return part


def copy_state(state):
    return [dict(p, arrays={k: v.copy() for k, v in p["arrays"].items()}, state=p["state"].copy()) for p in state]


def state_bytes(state):
    return b"".join(p["arrays"][n].tobytes() for p in state for n, _, _ in p["sections"]) + b"".join(p["state"].tobytes() for p in state)
