"""The DB-resident sweep of the split-f16 SC matcher (csrc/sc_match_e.hip, sc_match_e_kernel<true, 4, 4, false, true>): a workgroup holds
ONE DB group image in LDS and its four waves stream the query tiles of the query groups w, w + 4, ... of its query range - the present
sweep's roles exchanged.  Stage 1's MFMAs see the same operand bytes in the same order, so the distances must be the SAME BITS as the
present sweep's, whatever the shape: every case below runs two contexts in one process, PR_SC_SWEEP=q (present sweep) and PR_SC_SWEEP=d
(DB-resident), because `auto` keeps the present sweep at sizes this small.

Shapes: m in {9, 17, 33, 100} - a partial query group, query groups that are no multiple of four (idle waves), several fours of groups;
n in {1, 15, 16, 17, 257} - a group of one entry, a partial last group, exactly one full group, several workgroups.  With the binary path
on, channel 0 goes through the kernel on all eight XCDs (and the gate-2 launch behind the binary pass leaves at once); with
pr_set_sc_binary(ctx, 0) both channels go through it, four XCDs each.

Against the oracle the new form is held to the bound tests/test_gpu_parity.py applies to the split-f16 matchers (2e-6 on every
distance: test_sc_both_arithmetics_vs_oracle, test_sc_experiment_kernels_vs_oracle)."""
import numpy as np
import pytest

import oracle_lib
from so_dso_place_recognition_amd import synth

pytestmark = pytest.mark.gpu

MS = (9, 17, 33, 100)
NS = (1, 15, 16, 17, 257)
SPLIT_F16_TOL = 2e-6          # tests/test_gpu_parity.py: the split-f16 matchers against the oracle


@pytest.fixture(scope="module")
def sigs():
    db = synth.sc_database(71, max(NS) + 2)
    q, _ = synth.sc_queries(171, db, max(MS))
    for a in (db, q):
        a.setflags(write=False)
    return {"db": db, "q": q}


def _matcher(monkeypatch, sweep, binary, max_q, max_db, nsplit=None):
    """A Matcher whose context was created with PR_SC_SWEEP = sweep (the variable is read once, at pr_create)."""
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import Matcher
    monkeypatch.setenv("PR_SC_SWEEP", sweep)
    if nsplit is None:
        monkeypatch.delenv("PR_SC_NSPLIT", raising=False)
    else:
        monkeypatch.setenv("PR_SC_NSPLIT", str(nsplit))
    return Matcher("sc", max_q, max_db, ctx=api.Context(0, sc_binary=binary))


def _bits(mt, q):
    """Both distance matrices of pr_distances_dev for the queries q against the matcher's DB, as uint32."""
    import torch
    mt.local_phase1(torch.from_numpy(np.array(q)).cuda())
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(np.uint32).copy() for t in mt.distances())


def _both(monkeypatch, binary, nsplit=None, max_q=max(MS), max_db=max(NS) + 2):
    return (_matcher(monkeypatch, "q", binary, max_q, max_db, nsplit), _matcher(monkeypatch, "d", binary, max_q, max_db, nsplit))


def _same(a, b, label):
    for ch in (0, 1):
        assert a[ch].shape == b[ch].shape, label
        bad = np.argwhere(a[ch] != b[ch])
        assert bad.size == 0, f"{label}: channel {ch}, {len(bad)} of {a[ch].size} distances differ, first at {bad[0]}"


@pytest.mark.parametrize("binary", [True, False])
def test_same_bits_as_the_present_sweep(sigs, monkeypatch, binary):
    import torch
    mq, md = _both(monkeypatch, binary)
    for n in NS:
        dbd = torch.from_numpy(np.array(sigs["db"][:n])).cuda()
        mq.pack_database(dbd)
        md.pack_database(dbd)
        for m in MS:
            _same(_bits(mq, sigs["q"][:m]), _bits(md, sigs["q"][:m]), f"binary={binary} m={m} n={n}")
    mq.close()
    md.close()


@pytest.mark.parametrize("nsplit", [2, 3])
def test_same_bits_with_forced_query_ranges(sigs, monkeypatch, nsplit):
    """100 queries = 13 query groups = 4 fours: two and three query ranges (PR_SC_NSPLIT) cut them 2 + 2 and 1 + 1 + 2, the last range
    ragged (groups 8..12).  The reference is the present sweep at its own default geometry."""
    import torch
    mq = _matcher(monkeypatch, "q", False, 100, 259)
    md = _matcher(monkeypatch, "d", False, 100, 259, nsplit)
    dbd = torch.from_numpy(np.array(sigs["db"][:257])).cuda()
    mq.pack_database(dbd)
    md.pack_database(dbd)
    _same(_bits(mq, sigs["q"][:100]), _bits(md, sigs["q"][:100]), f"nsplit={nsplit}")
    mq.close()
    md.close()


def test_same_bits_with_zero_signatures(sigs, monkeypatch):
    """An all-zero signature on each side: packed as zeros, its distances are the NaN of the fix-up pass in both sweeps."""
    import torch
    db = sigs["db"][:100].copy()
    q = sigs["q"][:33].copy()
    db[37] = 0.0
    q[20] = 0.0
    for binary in (True, False):
        mq, md = _both(monkeypatch, binary)
        dbd = torch.from_numpy(db).cuda()
        mq.pack_database(dbd)
        md.pack_database(dbd)
        a, b = _bits(mq, q), _bits(md, q)
        _same(a, b, f"zero signatures, binary={binary}")
        d = b[0].view(np.float32)
        assert np.isnan(d[20]).all() and np.isnan(d[:, 37]).all() and not np.isnan(np.delete(np.delete(d, 20, 0), 37, 1)).any()
        mq.close()
        md.close()


def test_same_bits_on_an_appended_database(sigs, monkeypatch):
    """reserve_database with a capacity above the count, plus two appended rows: the channel stride of the DB image (the capacity's 63
    groups) is not the group count (17) the call walks."""
    import torch
    for binary in (True, False):
        mq, md = _both(monkeypatch, binary, max_db=1000)
        dbd = torch.from_numpy(np.array(sigs["db"][:259])).cuda()
        for mt in (mq, md):
            mt.reserve_database(dbd[:257])
            mt.append_database(dbd[257:258])
            mt.append_database(dbd[258:259])
            assert mt.n == 259
        _same(_bits(mq, sigs["q"][:33]), _bits(md, sigs["q"][:33]), f"appended DB, binary={binary}")
        mq.close()
        md.close()


def test_new_form_against_the_oracle(sigs, monkeypatch):
    import torch
    m, n = 40, 100
    q, db = sigs["q"][:m], sigs["db"][:n]
    rc, op, oi = oracle_lib.sc_distance(np.ascontiguousarray(q), np.ascontiguousarray(db))
    assert rc == 0
    md = _matcher(monkeypatch, "d", False, m, n)
    md.pack_database(torch.from_numpy(np.array(db)).cuda())
    gp, gi = (b.view(np.float32) for b in _bits(md, q))
    err = max(np.abs(gp - op).max(), np.abs(gi - oi).max())
    print(f"DB-resident sweep, {m} x {n}: max |d - oracle| = {err:.2e} (bound {SPLIT_F16_TOL:g})")
    assert err < SPLIT_F16_TOL
    md.close()


def test_whole_call_and_captured_replay(monkeypatch):
    """Matcher.match at 64 x 300, k = 5, mask 0 and 10: indices and scores bit-equal between the sweeps; a captured replay of the new
    form equals its stepwise call."""
    import torch
    from so_dso_place_recognition_amd.matcher import Matcher
    m, n, k = 64, 300, 5
    db = synth.sc_database(72, n)
    q, _ = synth.sc_queries(172, db, m)
    dbd, qd = torch.from_numpy(db).cuda(), torch.from_numpy(q).cuda()
    mq, md = _both(monkeypatch, True, max_q=m, max_db=n)
    mq.pack_database(dbd)
    md.pack_database(dbd)
    want = {}
    for mask in (0, 10):
        iq, sq = mq.match(qd, mask, 2.0, k)
        idd, sd = md.match(qd, mask, 2.0, k)
        torch.cuda.synchronize()
        assert torch.equal(iq, idd) and torch.equal(sq.view(torch.int64), sd.view(torch.int64)), f"mask {mask}"
        want[mask] = (idd.cpu().numpy().copy(), sd.cpu().numpy().copy())
    mq.close()
    md.close()
    monkeypatch.setenv("PR_SC_SWEEP", "d")
    mt = Matcher.on_new_stream("sc", m, n)
    with torch.cuda.stream(mt.stream):
        mt.pack_database(dbd)
        qs = qd.clone()
    torch.cuda.synchronize()
    cap = mt.capture(qs, 10, 2.0, k)
    idx, sc = cap.run(qd)
    assert np.array_equal(idx.cpu().numpy(), want[10][0]) and np.array_equal(sc.cpu().numpy().view(np.int64), want[10][1].view(np.int64))
    mt.close()
