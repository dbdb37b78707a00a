"""The M2DP all-pairs matchers bit for bit on exact inputs, at every tile edge and in every arithmetic.

tests/m2dp_match_cases.py draws signatures on a grid where the f16 split is exact, every product is exact and every partial sum fits 24
bits in any order, so the output of each arithmetic - split-f16 (m2dp_match_h_kernel<4, true>), single-product f16
(m2dp_match_h8_kernel<false>), fp32 MFMA (m2dp_match_kernel) - is determined bit for bit and a model in exact arithmetic predicts it
(tests/test_m2dp_match_cases_cpu.py shows that the inputs are exact and that a lost hi.lo' / lo.hi' product or a dropped variant pair
moves most outputs).  Every comparison below is on the uint32 bits of the full distance matrices of both channels.

Shapes: m in {1, 8, 9, 31, 32, 33, 97} - one query, a full / just exceeded query tile, a partial / full / just exceeded workgroup of 32 rows,
and 97: 13 tiles rounded up to 24, whose workgroups 4 .. 5 (per channel) hold padding tiles only and return at once;
n in {1, 7, 8, 9, 63, 64, 65, 449, 520, 1031} - partial DB tiles (n % 8), a partial / full / just exceeded sweep step of 8 tiles, and the
sizes at which the DB is cut into ranges: launch_m2dp_match_h clamps nsplit to DT8 / 4 with DT8 = ceil(ceil(n / 8) / 8), so the f16
kernels first split at n = 449 (DT8 = 8, two ranges); n = 520 gives DT8 = 9 (ranges 0..4 and 4..9), n = 1031 DT8 = 17 (four ranges, the
last one ragged).  launch_m2dp_match clamps to DT4 / 4 with DT4 = ceil(ceil(n / 8) / 4): the fp32 kernel first splits at n = 225 (DT4 = 8),
and 449, 520, 1031 give it 3, 4 and 8 ranges (DT4 = 15, 17, 33: ragged in all three), so no further n is needed for it.

Realistic values (test_realistic_values_against_the_oracle: synth rows with negated rows, per-block sign flips, entries of 1e-8 and exact
zeros, 33 x 520) against the fp64 oracle, measured on an MI355X: max |d - oracle| = 4.3e-7 (f16x2), 9.5e-5 (f16),
6.4e-7 (f32); the bounds are the project's own 1e-5 / 1e-3 / 1e-5.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import m2dp_match_cases as M
import m2dp_variant_child
import oracle_lib
from so_dso_place_recognition_amd import synth

pytestmark = pytest.mark.gpu

MS = (1, 8, 9, 31, 32, 33, 97)
NS = (1, 7, 8, 9, 63, 64, 65, 449, 520, 1031)
HOST_SHAPES = ((33, 65), (9, 520), (97, 1031))
GUARD = np.uint32(0x7FC0BEEF)          # a quiet NaN no distance can equal


@pytest.fixture(scope="module")
def want():
    """The model's distance matrices [2, 97, 1031] per arithmetic; every shape is the prefix [:, :m, :n]."""
    out = {a: M.expected(*M.cases(a), a) for a in M.ARITHS}
    for d in out.values():
        d.setflags(write=False)
    return out


def _matcher(arith, max_db=M.N_DB):
    from so_dso_place_recognition_amd import api
    from so_dso_place_recognition_amd.matcher import Matcher
    return Matcher("m2dp", M.N_Q, max_db, ctx=api.Context(0, sc_arith=arith))


def _dev(rows):
    import torch
    return torch.from_numpy(np.array(rows)).cuda()


def _run(mt, q):
    """Both distance matrices of pr_distances_dev for the query rows q against the matcher's DB, float32 on the host."""
    import torch
    mt.local_phase1(_dev(q))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in mt.distances())


def _check(got, want, m, n, label):
    msg = M.first_difference(got, want[:, :m, :n])
    assert msg is None, f"{label}, m={m} n={n}: {msg}"


@pytest.mark.parametrize("arith", M.ARITHS)
def test_model_bits_at_every_shape(want, arith):
    q, db = M.cases(arith)
    mt = _matcher(arith)
    for n in NS:
        mt.pack_database(_dev(db[:4 * n]))
        for m in MS:
            _check(_run(mt, q[:4 * m]), want[arith], m, n, arith)
    mt.close()


@pytest.mark.parametrize("arith", M.ARITHS)
def test_host_call_gives_the_same_bits(want, arith):
    """api.processM2DP (pr_m2dp_distance: host buffers, sets of its own) against the model, i.e. against the device path above."""
    from so_dso_place_recognition_amd import api
    q, db = M.cases(arith)
    ctx = api.Context(0, sc_arith=arith)
    for m, n in HOST_SHAPES:
        _check(api.processM2DP(q[:4 * m], db[:4 * n], ctx), want[arith], m, n, f"processM2DP {arith}")
    ctx.close()


@pytest.mark.parametrize("arith", M.ARITHS)
def test_float32_rows_give_the_same_bits(want, arith):
    """The pack kernels' float instantiation: every grid value has 14 significant bits, so its float32 is the same number."""
    q, db = (a.astype(np.float32) for a in M.cases(arith))
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip((q, db), M.cases(arith)))
    mt = _matcher(arith)
    for m, n in ((33, 65), (9, 520)):
        mt.pack_database(_dev(db[:4 * n]))
        _check(_run(mt, q[:4 * m]), want[arith], m, n, f"{arith}, float32 rows")
    mt.close()


@pytest.mark.parametrize("arith", M.ARITHS)
def test_unit_family_gives_its_listed_values(arith):
    """One-hot rows and an all-zero signature on each side: S is 0, +-65536 or +-131072, so d is one of 0.5, 0, -0.5, 1, 1.5 exactly and
    0.5 in the zero signature's row and column; then one-hot queries against grid rows and grid queries against the one-hot DB."""
    uq, udb = M.unit_family()
    gq, gdb = M.cases(arith)
    mt = _matcher(arith)
    mt.pack_database(_dev(udb))
    got = np.stack(_run(mt, uq))
    assert np.isin(got, M.UNIT_VALUES).all()
    assert (got[:, M.UNIT_ZERO_Q] == 0.5).all() and (got[:, :, M.UNIT_ZERO_DB] == 0.5).all()
    for ch in (0, 1):
        assert set(np.unique(got[ch])) == set(M.UNIT_VALUES)
    msg = M.first_difference(got, M.expected(uq, udb, arith))
    assert msg is None, f"unit family, {arith}: {msg}"
    msg = M.first_difference(_run(mt, gq[:4 * 33]), M.expected(gq[:4 * 33], udb, arith))
    assert msg is None, f"grid queries against the unit DB, {arith}: {msg}"
    mt.pack_database(_dev(gdb[:4 * 65]))
    msg = M.first_difference(_run(mt, uq), M.expected(uq, gdb[:4 * 65], arith))
    assert msg is None, f"unit queries against grid rows, {arith}: {msg}"
    mt.close()


@pytest.mark.parametrize("arith", M.ARITHS)
def test_bits_do_not_depend_on_the_history_of_the_buffers(want, arith):
    """One matcher, n walked down and then up, m walked down inside each n: every call after the first finds, in the unused part of its
    last tile (and of its query tiles), whatever an earlier, larger call left there or the set's own clearing put there."""
    q, db = M.cases(arith)
    mt = _matcher(arith)
    for n in NS[::-1] + NS[1:]:
        mt.pack_database(_dev(db[:4 * n]))
        for m in MS[::-1]:
            _check(_run(mt, q[:4 * m]), want[arith], m, n, f"{arith}, reused buffers")
    mt.close()


@pytest.mark.parametrize("arith", ["f16x2", "f16"])
def test_same_bits_on_an_appended_database(want, arith):
    """reserve_database at capacity 1200 with the first 1029 signatures, then two appends of one signature each: the channel stride DTS
    (150 tiles) is not the tile count DT (129) the call walks, and the appends land in the middle of the last tile."""
    q, db = M.cases(arith)
    mt = _matcher(arith, max_db=1200)
    dbd = _dev(db)
    mt.reserve_database(dbd[:4 * 1029])
    mt.append_database(dbd[4 * 1029:4 * 1030])
    mt.append_database(dbd[4 * 1030:4 * 1031])
    assert mt.n == 1031
    for m in (97, 33):
        _check(_run(mt, q[:4 * m]), want[arith], m, 1031, f"{arith}, appended DB")
    mt.close()


@pytest.mark.parametrize("arith", M.ARITHS)
def test_rows_around_the_matrices_stay_untouched(want, arith):
    """pr_distances_dev into tensors of the test's own with one row of a pattern in front of and one behind each [m, n] matrix: the
    kernels' store range (the buffer descriptor `rd`, the fp32 kernel's row test) ends with query row m - 1."""
    import torch
    q, db = M.cases(arith)
    mt = _matcher(arith)
    for n in (65, 520):
        mt.pack_database(_dev(db[:4 * n]))
        for m in (31, 33, 97):
            mt.local_phase1(_dev(q[:4 * m]))
            bufs = [torch.from_numpy(np.full((m + 2, n), GUARD, np.uint32).view(np.float32)).cuda() for _ in (0, 1)]
            ptrs = [C.c_void_p(b.data_ptr() + 4 * n) for b in bufs]
            mt.ctx.check(mt.lib.pr_distances_dev(mt.ctx.h, mt.q, mt.db, *ptrs))
            torch.cuda.synchronize()
            got = [b.cpu().numpy() for b in bufs]
            for ch in (0, 1):
                rows = got[ch].view(np.uint32)
                assert (rows[0] == GUARD).all(), f"{arith} m={m} n={n}: channel {ch}, the row in front of the matrix was written"
                assert (rows[m + 1] == GUARD).all(), f"{arith} m={m} n={n}: channel {ch}, row m was written"
            _check([g[1:m + 1] for g in got], want[arith], m, n, f"{arith}, guarded")
    mt.close()


def _realistic():
    """synth's M2DP rows (all positive, entries in a 6:1 band) made to look like singular vectors: negated rows, one variant row per
    signature with the sign of one block per channel flipped, entries at 1e-8 of the row's scale, exact zeros."""
    rng = np.random.default_rng(5)

    def renorm(a):
        r = a.reshape(-1, 2, 192)
        r[..., :64] /= np.sqrt((r[..., :64] ** 2).sum(-1, keepdims=True))
        r[..., 64:] /= np.sqrt((r[..., 64:] ** 2).sum(-1, keepdims=True))

    def rough(a, tiny_share, zero_share):
        a[rng.random(a.shape[0]) < 0.5] *= -1.0                                   # whole rows negated
        sig = a.reshape(-1, 4, 2, 192)
        for s in range(sig.shape[0]):
            v, first = int(rng.integers(4)), bool(rng.integers(2))
            sig[s, v, :, :64] *= -1.0 if first else 1.0
            sig[s, v, :, 64:] *= 1.0 if first else -1.0
        a[rng.random(a.shape) < tiny_share] *= 1e-8
        renorm(a)
        a[rng.random(a.shape) < zero_share] = 0.0

    db = synth.m2dp_database(43, 520)
    rough(db, 0.2, 0.01)
    q, _ = synth.m2dp_queries(44, db, 33)                                         # copies of the roughened rows + noise
    rough(q, 0.05, 0.01)
    return q, db


def test_realistic_values_against_the_oracle():
    from so_dso_place_recognition_amd import api
    q, db = _realistic()
    assert (db < 0).any() and (db == 0).any() and ((np.abs(db) < 1e-6) & (db != 0)).any()
    rc, op, oi = oracle_lib.m2dp_distance(q, db)
    assert rc == 0
    assert op.min() < -0.3 and op.max() > 0.5                                     # near-copies, and pairs whose 16 variant dots are all negative
    errs = {}
    for arith in M.ARITHS:
        mt = _matcher(arith)
        mt.pack_database(_dev(db))
        gp, gi = _run(mt, q)
        mt.close()
        errs[arith] = max(np.abs(gp - op).max(), np.abs(gi - oi).max())
        print(f"realistic 33 x 520, {arith}: max |d - oracle| = {errs[arith]:.3e}")
    assert errs["f16x2"] < 1e-5 and errs["f32"] < 1e-5                            # tests/test_gpu_parity.py
    assert errs["f16"] < 1e-3                                                     # tests/test_gpu_f16.py


def test_ab_switches_give_the_model_bits(want, tmp_path):
    """PR_M2_QTB=3 (three query tiles per workgroup, split-f16), PR_M2_WAVES=8 (the eight-wave split-f16 kernel) and PR_M2_WAVES=4 (the
    four-wave single-product kernel): function-static getenv()s, so each runs in a child process (tests/m2dp_variant_child.py), one after
    the other; the first child that fails ends the test and no further child is started."""
    child = os.path.abspath(m2dp_variant_child.__file__)
    for var, value, arith in (("PR_M2_QTB", "3", "f16x2"), ("PR_M2_WAVES", "8", "f16x2"), ("PR_M2_WAVES", "4", "f16")):
        env = {k: v for k, v in os.environ.items() if k not in ("PR_M2_QTB", "PR_M2_WAVES")}
        env[var] = value
        out = str(tmp_path / f"{var}_{value}_{arith}.npz")
        r = subprocess.run([sys.executable, child, arith, out], env=env, timeout=120, capture_output=True, text=True)
        assert r.returncode == 0, f"{var}={value} {arith}: the child left with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        res = np.load(out)
        for m, n in m2dp_variant_child.SHAPES:
            _check((res[f"p_{m}_{n}"], res[f"i_{m}_{n}"]), want[arith], m, n, f"{var}={value} {arith}")
