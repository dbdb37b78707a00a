"""m2dp_svd_kernel where the leading singular pair is tied, nearly tied, slow to separate or degenerate, and the list of named rows.

The cases (m2dp_svd_cases.py, checked on the CPU by test_m2dp_svd_cases_cpu.py) go through pr_m2dp_generate_frames_dev on hand-made frames, so the
bin matrices on the device are the oracle's and only the singular pairs are in question.  Per (variant, channel) matrix, from LAPACK:
  s1/s2 >= 1.03, rank 1 or zero : the pair is unique; the row is never named and is the oracle's within 1e-9 (the project's M2DP tolerance);
  s1/s2 <= 1.01                 : the row is always named (PR_WARN_M2DP_SVD, pr_m2dp_svd_rows), exact ties included;
  in between (grey)             : either.
A named row is not compared with the oracle (whose Jacobi sweeps also end on some vector of the tied span) but must be usable: u a unit vector
inside the span of the tied group's left singular vectors, sum(u) >= 0, v = A^T u / ||A^T u||.

Measured on an MI355X, max |device - oracle| per family of unique pairs of the mixed batch (bound 1e-9): s1/s2 >= 1.05 3.3e-15, 1.03 <= s1/s2 <
1.05 2.1e-13, grey rows that converged 2.9e-13, rank 1 and zero exact; of the three grey rows the one at 1.015 is named.  Before the kernel's
trace test the six exact-tie rows of the mixed batch came back unnamed (the near-tie rows were named): test_mixed_batch failed on them."""
import numpy as np
import pytest

import m2dp_svd_cases as S

pytestmark = pytest.mark.gpu

TOL = 1e-9                    # the project's M2DP tolerance (test_gpu_gen_edges.py, __graft_entry__.smoke)


@pytest.fixture(scope="module")
def api():
    from so_dso_place_recognition_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    """a context of this module's own: its warning bits stay out of the default context other modules assert on"""
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return S.all_cases()


def _generate(ctx, batch, have_ave=1):
    """pr_m2dp_generate_frames_dev over the clouds of `batch` with their hand-made frames -> [len(batch), 4, 384]"""
    import torch
    xyz = np.concatenate([c.xyz for c in batch])
    inten = np.concatenate([c.inten for c in batch])
    offs = np.concatenate([[0], np.cumsum([len(c.xyz) for c in batch])]).astype(np.int64)
    frames = np.stack([c.frame for c in batch]).copy()
    if not have_ave:
        frames[:, 14:] = 0.0                               # the call computes the averages itself
    dx, di, do, df = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xyz, inten, offs, frames))
    N = len(batch)
    out = torch.full((N * 4, 384), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.pr_m2dp_generate_frames_dev(ctx.h, dx.data_ptr(), di.data_ptr(), do.data_ptr(), N, batch[0].max_rho, df.data_ptr(), have_ave,
                                                  out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy().reshape(N, 4, 384)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _named(api, ctx):
    """the named rows of the last call; ascending and without duplicates, whatever else a test asserts"""
    rows = [int(r) for r in api.m2dp_svd_rows(ctx)]
    assert rows == sorted(set(rows)), rows
    return rows


@pytest.fixture(scope="module")
def spans(cases):
    """{(name, v, ch): left singular vectors of the tied group (LAPACK)} for the tied, near-tied and grey matrices"""
    out = {}
    for c in cases:
        for v in range(4):
            for ch in range(2):
                if c.band[v][ch] in S.UNRESOLVED:
                    out[c.name, v, ch] = np.linalg.svd(c.mats[v, ch])[0][:, :S.tied_group(c.sv[v][ch])]
    return out


def _check_unique(c, v, ch, g, worst):
    err = np.abs(g - c.rows[v, 192 * ch:192 * ch + 192]).max()
    worst[c.band[v][ch]] = max(worst.get(c.band[v][ch], 0.0), err)
    assert err < TOL, (c.name, v, ch, c.band[v][ch], c.ratio[v][ch], err)


def _check_valid(c, v, ch, g, spans):
    """a named row's channel whose own matrix is tied, near-tied or grey"""
    A = c.mats[v, ch]
    u, vv = g[:64], g[64:]
    tag = (c.name, v, ch, c.band[v][ch], c.ratio[v][ch])
    assert np.isfinite(g).all(), tag
    assert abs(np.linalg.norm(u) - 1) < 1e-12, (tag, np.linalg.norm(u) - 1)
    assert u.sum() >= 0, (tag, u.sum())
    U = spans[c.name, v, ch]
    out = np.linalg.norm(u - U @ (U.T @ u))
    assert out < TOL, (tag, out)
    w = A.T @ u
    w = w / np.linalg.norm(w)
    assert np.abs(vv - w).max() < TOL, (tag, np.abs(vv - w).max())


def _check_batch(batch, got, named, spans, worst):
    """every row of a batch against what its class allows; returns (truth, grey)"""
    truth, grey = S.expected_rows(batch)
    assert truth <= set(named), ("rows at s1/s2 <= 1.01 that are not named", sorted(truth - set(named)))
    assert set(named) <= truth | grey, ("named rows with a unique pair", sorted(set(named) - truth - grey))
    for i, c in enumerate(batch):
        for v in range(4):
            for ch in range(2):
                g = got[i, v, 192 * ch:192 * ch + 192]
                if 4 * i + v in named and c.band[v][ch] in S.UNRESOLVED:
                    # (the list names rows, not channels: a grey channel that converged beside a tied one gets the validity check only, not
                    # the 1e-9 oracle bound.  No case has such a row today - every grey matrix shares its row with unique ones only; whoever
                    # adds one must decide that channel's check here, or it silently gets the weaker one)
                    _check_valid(c, v, ch, g, spans)
                else:                                       # unnamed (clean, or a grey row that converged), or a named row's unique channel
                    _check_unique(c, v, ch, g, worst)
    return truth, grey


# ------------------------------------------------------------------------------------------------ one mixed batch of all cases
@pytest.mark.parametrize("have_ave", [1, 0])
def test_mixed_batch(api, ctx, cases, spans, have_ave):
    ctx.take_warnings()
    got = _generate(ctx, cases, have_ave)
    named = _named(api, ctx)
    worst = {}
    truth, grey = _check_batch(cases, got, named, spans, worst)
    assert ctx.take_warnings() & 2
    ties = {4 * i + v for i, c in enumerate(cases) for v in range(4) if "tie" in c.band[v]}
    print(f"have_ave {have_ave}: named {named}; exact-tie rows {sorted(ties)}; grey rows named {sorted(grey & set(named))} of {sorted(grey)}")
    print("max |device - oracle| per family (bound 1e-9): " + ", ".join(f"{k} {e:.2e}" for k, e in sorted(worst.items())))
    assert {"slow", "well", "rank1", "zero"} <= set(worst)


# ------------------------------------------------------------------------------------------------ batch offsets
def test_row_numbers_past_the_first_scratch_batches(api, ctx, cases, spans):
    """600 clouds = three scratch batches of 256 on two streams (c0 = 0, 256, 512): tie cases at the edges of every batch, clouds that cannot
    be named everywhere else.  The named list is exactly the expected rows, and every row has the bits a small batch gives it"""
    ctx.take_warnings()
    fill = S.clean_cases()
    N = 600
    spots = {0: "tie_a", 100: "near_004", 255: "tie3_a", 256: "tie_c", 300: "near_0075", 511: "tie_b", 512: "near_00007", 550: "tie3_b",
             N - 1: "slow_tie"}
    batch = [S.by_name(spots[i]) if i in spots else fill[i % len(fill)] for i in range(N)]
    truth, grey = S.expected_rows(batch)
    assert not grey and len(truth) >= len(spots) and {r // 4 for r in truth} == set(spots)
    distinct = list({c.name: c for c in batch}.values())
    small = dict(zip([c.name for c in distinct], _generate(ctx, distinct)))
    small_named = _named(api, ctx)
    assert set(small_named) == S.expected_rows(distinct)[0]
    got = _generate(ctx, batch)
    named = _named(api, ctx)
    assert named == sorted(truth), (sorted(set(named) - truth), sorted(truth - set(named)))
    assert ctx.take_warnings() & 2
    for i, c in enumerate(batch):
        assert np.array_equal(_bits(got[i]), _bits(small[c.name])), (i, c.name)
    _check_batch(distinct, np.stack([small[c.name] for c in distinct]), small_named, spans, {})


# ------------------------------------------------------------------------------------------------ the list belongs to the last call
def test_list_is_the_last_calls_and_argument_forms(api, ctx, cases):
    from so_dso_place_recognition_amd import _lib
    ctx.take_warnings()
    ties = [S.by_name(n) for n in ("tie_a", "near_001", "tie3_a", "slow_tie")]
    _generate(ctx, ties)
    want = sorted(S.expected_rows(ties)[0])
    assert len(want) >= 4 and _named(api, ctx) == want
    fn = ctx.lib.pr_m2dp_svd_rows
    cnt = np.full(1, -7, np.int32)
    assert fn(ctx.h, None, 0, cnt.ctypes.data) == _lib.PR_OK and cnt[0] == len(want)         # cap = 0, rows = NULL: the count
    rows = np.full(8, -7, np.int32)
    cnt[0] = -7
    assert fn(ctx.h, rows.ctypes.data, 2, cnt.ctypes.data) == _lib.PR_OK                      # a cap below the count: cap rows, the full count
    assert cnt[0] == len(want) and list(rows[:2]) == want[:2] and (rows[2:] == -7).all()
    assert fn(ctx.h, rows.ctypes.data, 8, None) == _lib.PR_EINVAL                             # count = NULL
    assert fn(ctx.h, None, 4, cnt.ctypes.data) == _lib.PR_EINVAL                              # rows = NULL with a cap
    clean = S.clean_cases()
    got = _generate(ctx, clean)
    assert _named(api, ctx) == []                                                             # the clean call's list, not the one before
    for c, g in zip(clean, got):
        assert np.abs(g - c.rows).max() < TOL, c.name
    assert ctx.take_warnings() & 2                                                            # the bit of the first call stays until taken
    assert not (ctx.take_warnings() & 2)
    _generate(ctx, clean)
    assert _named(api, ctx) == [] and not (ctx.take_warnings() & 2)


# ------------------------------------------------------------------------------------------------ more pairs than the record holds
def test_more_pairs_than_the_record_holds(api, ctx, cases, spans):
    """tie_a ties both channels of one row: 550 copies are 1100 (row, channel) pairs for 1024 slots"""
    ctx.take_warnings()
    c = S.by_name("tie_a")
    pairs = sum(c.band[v][ch] in ("tie", "near") for v in range(4) for ch in range(2))
    N = 550
    assert pairs * N > 1024
    batch = [c] * N
    got = _generate(ctx, batch)                                                               # (ctx.check: PR_OK)
    named = _named(api, ctx)
    truth, _ = S.expected_rows(batch)
    assert ctx.take_warnings() & 2
    assert 0 < len(named) <= 1024 and set(named) <= truth, (len(named), sorted(set(named) - truth)[:8])
    assert len(named) >= 1024 // pairs                                                        # (1024 recorded pairs name at least that many rows)
    assert np.isfinite(got).all()
    for i in range(1, N):
        assert np.array_equal(_bits(got[i]), _bits(got[0])), i
    mixed = [S.by_name(n) for n in ("slow_a", "tie_b", "far", "near_0007", "flat", "tie3_b")]
    got = _generate(ctx, mixed)
    named = _named(api, ctx)
    assert not S.expected_rows(mixed)[1] and named == sorted(S.expected_rows(mixed)[0])      # the record buffer is intact
    _check_batch(mixed, got, named, spans, {})
    assert ctx.take_warnings() & 2


# ------------------------------------------------------------------------------------------------ repeatability
def test_mixed_batch_twice_gives_the_same_bits(api, ctx, cases):
    ctx.take_warnings()
    a = _generate(ctx, cases)
    na = _named(api, ctx)
    b = _generate(ctx, cases)
    nb = _named(api, ctx)
    assert na == nb and len(na) > 0
    assert np.array_equal(_bits(a), _bits(b))
    ctx.take_warnings()
