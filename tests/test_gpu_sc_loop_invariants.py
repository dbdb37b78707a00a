"""What the split-f16 SC matcher (csrc/sc_match_e.hip) keeps across the units of a wave's DB sweep instead of fetching or computing it per
unit: the stage-2 constants, resident in AccVGPRs, and one base register per operand pair of the 16-byte aligned query image (csrc/kernels.hpp:
sch_qrow_byte), which the single-product kernel of the binary intensity channel gathers its compact LDS image from.  A constant or base
clobbered after a wave's first unit, a wrong tile address in the layout or a mis-sized LDS image shows at small sizes: 1405 signatures = 88
DB groups, the last one ragged, so the waves of every launch form run several units, and the query counts walk through every
instantiation - sc_match_e_kernel<true, 4, 1 | 2 | 4>, <false, 8, 1 | 2 | 4 | 8, true> (binary intensity channel) and
<false, 8, 1 | 2 | 4 | 8> (PR_SC_ARITH_F16).

Bounds.  Split-f16 arithmetic, with or without the binary path: top-k indices exact, scores within helpers.score_tol, every distance
within 1e-5 of the oracle (the bound of tests/test_gpu_binary.py and of smoke()).  The single-product arithmetic PR_SC_ARITH_F16 keeps
10 bits of every factor, so its distances carry ~3e-5 of noise and cannot meet 1e-5 whatever the kernel does: that mode is held to the
bounds the suite already has for it (tests/test_gpu_f16.py: distances within 1e-3, scores within 3e-2 + 1e-3 |score|), indices exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import oracle_lib
from so_dso_place_recognition_amd import synth

N = 1400 + 5                # 88 DB groups of 16, the last one holds 13 entries
MS = (1, 8, 12, 16, 24, 40, 72)
K = 3
# the binary launch of this size walks 8 ranges of 11 groups (the split-f16 launch of a two-channel call 4 ranges of 22): entries in the
# first, a middle and the last group of a range - groups 0 and 11, 5 and 49, 10, 21 and the ragged 87
TARGETS = np.array([3, 11 * 16 + 5, 5 * 16 + 5, 49 * 16 + 9, 10 * 16 + 15, 21 * 16, N - 1])


@pytest.fixture(scope="module")
def case():
    """DB, 72 queries planted on TARGETS, and the oracle's distances and top-3 of all of them (a row's answer does not depend on the
    other queries of a call, so every query count takes its first m rows)."""
    db = synth.sc_database(45, N)
    q, et = synth.sc_queries(47, db[TARGETS], max(MS))
    planted = TARGETS[et]
    assert set(planted) == set(TARGETS) and set(planted[:8]) >= {3, N - 1}, planted[:8]    # (of this seed: every place is hit, the first and the last entry by the first 8 queries)
    rc, dp, di = oracle_lib.sc_distance(q, db)
    assert rc == 0
    rc, oidx, osc = oracle_lib.match_topk(0, q, db, 0, 2.0, K)
    assert rc == 0 and np.array_equal(oidx[:, 0], planted)
    for a in (db, q, dp, di, oidx, osc):
        a.setflags(write=False)
    return {"db": db, "q": q, "dp": dp, "di": di, "oidx": oidx, "osc": osc}


def _ctx(mode):
    from so_dso_place_recognition_amd import api
    if mode == "binary":
        return api.Context(0)
    if mode == "split":
        return api.Context(0, sc_binary=False)
    return api.Context(0, sc_arith="f16")


def _check(case, rows, idx, sc, dp, di, mode, label):
    """rows: the queries of `case` this call answered (slice or index array)."""
    odp, odi, oidx, osc = case["dp"][rows], case["di"][rows], case["oidx"][rows], case["osc"][rows]
    if mode == "f16":
        dtol, stol = 1e-3, 3e-2 + 1e-3 * np.abs(osc)
    else:
        dtol, stol = 1e-5, helpers.score_tol(osc, helpers.row_sigmas(odp, odi))
    derr = max(np.abs(dp - odp).max(), np.abs(di - odi).max())
    serr = (np.abs(sc - osc) / stol).max()
    print(f"{label}: max |d - oracle| = {derr:.2e} (bound {dtol:g}), max |score - oracle| / tolerance = {serr:.3f}")
    assert np.array_equal(idx, oidx), label
    assert serr <= 1.0, label
    assert derr < dtol, label


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("mode", ["binary", "split", "f16"])
def test_topk_and_every_distance_against_the_oracle(case, mode, m):
    import torch
    from so_dso_place_recognition_amd.matcher import Matcher
    mt = Matcher("sc", m, N, ctx=_ctx(mode))
    mt.pack_database(torch.from_numpy(case["db"]).cuda())
    idx, sc = mt.match(torch.from_numpy(case["q"][:m]).cuda(), 0, 2.0, K)
    dp, di = (t.cpu().numpy() for t in mt.distances())
    if mode == "binary":      # the single-product launch with integer rounding answered channel 1
        st = C.c_int32(-1)
        mt.ctx.check(mt.lib.pr_sc_binary_state(mt.ctx.h, mt.q, mt.db, C.byref(st)))
        assert st.value == 1
    _check(case, slice(0, m), idx.cpu().numpy(), sc.cpu().numpy(), dp, di, mode, f"{mode} m={m}")
    mt.close()


@pytest.mark.gpu
def test_appended_database_has_the_capacitys_channel_stride(case):
    """reserve_database + append_database: the DB image is laid out for 2000 entries (125 groups per channel), the call walks 88."""
    import torch
    from so_dso_place_recognition_amd.matcher import Matcher
    m = 24
    mt = Matcher("sc", m, 2000, ctx=_ctx("binary"))
    dbd = torch.from_numpy(case["db"]).cuda()
    mt.reserve_database(dbd[:1000])
    mt.append_database(dbd[1000:1399])
    mt.append_database(dbd[1399:])
    assert mt.n == N
    idx, sc = mt.match(torch.from_numpy(case["q"][:m]).cuda(), 0, 2.0, K)
    dp, di = (t.cpu().numpy() for t in mt.distances())
    _check(case, slice(0, m), idx.cpu().numpy(), sc.cpu().numpy(), dp, di, "binary", "appended DB m=24")
    mt.close()


@pytest.mark.gpu
def test_captured_graph_replayed_twice(case):
    import torch
    from so_dso_place_recognition_amd.matcher import Matcher
    m = 12
    mt = Matcher.on_new_stream("sc", m, N)
    with torch.cuda.stream(mt.stream):
        mt.pack_database(torch.from_numpy(case["db"]).cuda())
        qs = torch.from_numpy(case["q"][:m]).cuda()
    cap = mt.capture(qs, 0, 2.0, K)
    for r in (1, 2):          # queries 12..23, then 24..35, through the same graph
        rows = slice(r * m, (r + 1) * m)
        idx, sc = cap.run(torch.from_numpy(case["q"][rows]).cuda())
        dp, di = (t.cpu().numpy() for t in mt.distances())
        _check(case, rows, idx.cpu().numpy(), sc.cpu().numpy(), dp, di, "binary", f"graph replay {r}")
    mt.close()


# vgpr_spill_count of the sc_match_e_kernel<false, ...> instantiations at the parent commit f9102b9 (hipcc -O3, gfx950), by (NQG, SV)
PARENT_SPILLS = {(1, False): 0, (2, False): 0, (4, False): 0, (8, False): 0, (1, True): 0, (2, True): 0, (4, True): 0, (8, True): 0}


def test_kernel_builds_without_new_spills(tmp_path):
    """The resident constants and the deeper DB ring must fit the registers: no spill in any split-f16 instantiation, none beyond the
    parent's in the single-product ones (two waves per SIMD, up to 253 of 256 registers in use)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "sc_match_e.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        os.path.join(root, "so_dso_place_recognition_amd", "csrc", "sc_match_e.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    found = {}
    for name, spills in re.findall(r"\.name:\s+(\S*sc_match_e_kernel\S*)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text):
        mt = re.search(r"sc_match_e_kernelILb([01])ELi(\d)ELi(\d)ELb([01])E", name)
        found[(mt.group(1) == "1", int(mt.group(3)), mt.group(4) == "1")] = int(spills)
    assert {k for k in found if k[0]} == {(True, 1, False), (True, 2, False), (True, 4, False)}, sorted(found)
    assert {(k[1], k[2]) for k in found if not k[0]} == set(PARENT_SPILLS), sorted(found)
    for (lo, nqg, sv), spills in sorted(found.items()):
        assert spills <= (0 if lo else PARENT_SPILLS[(nqg, sv)]), (lo, nqg, sv, spills)
