"""The sequence matcher (pr_seq_select_dev, pr_seqmatch) without a device: the text of the rule in the header, the ABI
surface, the argument errors that are returned before any device is touched, api.seq_steps, and properties of the NumPy restatement
the GPU tests compare the kernels with (seqmatch_np.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import oracle_lib
import seqmatch_np as sq
from so_dso_place_recognition_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NAMES = ("pr_seq_select_dev", "pr_seq_tile", "pr_match_topk_seq_f64", "pr_seqmatch_create", "pr_seqmatch_push_dev", "pr_seqmatch_push",
         "pr_seqmatch_reset", "pr_seqmatch_read", "pr_seqmatch_scratch_bytes", "pr_seqmatch_destroy")


def test_seq_header_states_the_rule():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for words in ("DESIGN.md 4.23", "steps[v][0] == 0", "how many DB rows BEHIND the candidate", "no velocity arithmetic happens there",
                  "f(i, j) = p_weight * (((double)d_p[i][j] - mean_p) / sd_p) + ((double)d_i[i][j] - mean_i) / sd_i",
                  "sd = sqrt(M2 / (count - 1.0))", "With d_i == NULL there is no normalisation: f = (double)d_p[i][j]",
                  "|(q_row0 + a) - (db_row0 + c)| < mask_width", "L_i = min(L, i + 1)", "A query shard does not see earlier shards",
                  "added in ascending l from 0.0, of f(i - l, j - steps[v][l])", "+/-Inf terms add by IEEE", "or the sum is NaN",
                  "strict <, so the first v wins a tie", "its d_S entry is +Inf", "the k smallest candidates by (S, j)",
                  "idx = db_row0 + j, score = S, vel = v", "Missing slots are -1 / NaN / -1", "NO fp64 re-evaluation and NO containment",
                  "every grid\n *                       depends on (m, n) only", "The ring, the row ids\n *      and the counter do not change by a byte",
                  "n = count clamped into 0 .. capacity", "added in ascending c from 0.0", "The order of both sums is fixed by n alone",
                  "p[t] += p[t + s] for s = 128, 64, .. 1", "normalize = 0 needs channels == 1", "the counter\n *      is committed by one thread",
                  "L_n = min(L, pushes so far including this one)", "0 <= c < n_l and |n_l - c| >= mask_width",
                  "over j < n with n - j >= mask_width", "info = {pushed, L_n, pushes after, 0}", "still counts as a push"):
        assert words in txt, words


def test_seq_symbols_bindings_and_build():
    txt = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[n][1]), n              # the argument counts of the bindings are the header's
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("pr_seq")) + ["pr_match_topk_seq_f64"] == sorted(NAMES[:2] + NAMES[3:]) + [NAMES[2]]
    for name, val in (("PR_SEQ_MAX_L", 32), ("PR_SEQ_MAX_V", 16), ("PR_SEQ_MAX_STEP", 64), ("PR_SEQ_MAX_K", 32), ("PR_SEQMATCH_MAX_K", 128)):
        assert f"#define {name} {val}\n" in code, name
    assert (_lib.SEQ_MAX_L, _lib.SEQ_MAX_V, _lib.SEQ_MAX_STEP, _lib.SEQ_MAX_K, _lib.SEQMATCH_MAX_K) == (32, 16, 64, 32, 128)
    assert (sq.MAX_L, sq.MAX_V, sq.MAX_STEP, sq.MAX_K, sq.ONLINE_MAX_K) == (32, 16, 64, 32, 128)
    R, W = api.seq_tile()
    assert R >= 2 and W >= 64 and W % 64 == 0
    for m_ in ("push_torch", "push", "reset", "read", "close"):
        assert hasattr(api.SequenceFilter, m_), m_
    from so_dso_place_recognition_amd.matcher import Matcher
    assert hasattr(Matcher, "match_sequence") and hasattr(api, "seq_select_torch") and hasattr(api, "match_topk_seq")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"seqmatch\.o: seqmatch\.hip[^\n]*\n\t\$\(HIPCC\) \$\(GENFLAGS\)", mk) and "-ffp-contract=off" in mk
    hip = open(os.path.join(CSRC, "seqmatch.hip")).read()
    assert "atomic" not in hip.replace("No atomics", "")                                  # selection by (score, index) is order-free


def scratch_bytes(cap, ch, V, L, K):
    """the formula of the header"""
    if not (1 <= cap <= 1 << 24 and ch in (1, 2, 4) and 1 <= V <= 16 and 1 <= L <= 32 and 1 <= K <= 128):
        return 0
    r = lambda b: (b + 15) & ~15
    B = (cap + 255) // 256
    return (r(8 * L * cap) + r(4 * L) + 16 + 64 + 16 + r(4 * V * L) + r(8 * B * K) + 2 * r(4 * B * K)) + (r(8 * ch * cap) + 16 + r(8 * K) + 2 * r(4 * K) + 16)


def test_seqmatch_scratch_size_formula():
    lib = _lib.load()
    for case in ((4096, 2, 6, 8, 8), (1, 1, 1, 1, 1), (1 << 24, 4, 16, 32, 128), (257, 4, 3, 5, 7), (3475, 1, 2, 32, 128)):
        want = scratch_bytes(*case)
        assert want > 8 * case[0] * case[3] and lib.pr_seqmatch_scratch_bytes(*case) == want, case
    for bad in ((0, 1, 1, 1, 1), ((1 << 24) + 1, 1, 1, 1, 1), (8, 3, 1, 1, 1), (8, 1, 0, 1, 1), (8, 1, 17, 1, 1), (8, 1, 1, 0, 1), (8, 1, 1, 33, 1),
                (8, 1, 1, 1, 0), (8, 1, 1, 1, 129)):
        assert lib.pr_seqmatch_scratch_bytes(*bad) == 0 == scratch_bytes(*bad), bad


def test_seq_select_argument_errors():
    """every PR_EINVAL of the batch call fires with ctx == NULL: no device is touched (the addresses are never dereferenced)"""
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    store = (C.c_double * 8)()
    a = C.addressof(store)

    def call(d_p=a, d_i=a, m=4, n=4, mom=a, steps=a, V=2, L=3, mw=0, k=1, idx=a, score=a, vel=a):
        rc = lib.pr_seq_select_dev(None, d_p, d_i, m, n, mom, steps, V, L, 0, 0, mw, 2.0, k, idx, score, vel, None)
        assert rc == _lib.PR_EINVAL
        return err()

    for name in ("d_p", "steps", "idx", "score", "vel"):
        assert "a required pointer is NULL" in call(**{name: None}), name
    assert "mom is NULL with d_i given" in call(mom=None)
    assert "m=-1" in call(m=-1) and "n=0" in call(n=0)
    for V in (0, 17):
        assert "V=%d outside" % V in call(V=V)
    for L in (0, 33):
        assert "L=%d outside" % L in call(L=L)
    for k in (0, 33):
        assert "k=%d outside" % k in call(k=k)
    assert "mask_width=-1 is negative" in call(mw=-1)
    assert "ctx is NULL" in call()
    assert lib.pr_match_topk_seq_f64(None, 0, None, 0, None, 0, 0, 2.0, 1, None, 1, 1, None, None, None) == _lib.PR_EINVAL


def test_seqmatch_create_argument_errors():
    lib = _lib.load()
    err = lambda: lib.pr_last_error(None).decode()
    good = np.array([[0, 1, 2], [0, -1, -2]], np.int32)

    def create(cap=16, ch=2, steps=good, V=None, L=None, max_k=4, out=True):
        h = C.c_void_p(1)
        st = None if steps is None else np.ascontiguousarray(steps, np.int32)
        V = V if V is not None else (st.shape[0] if st is not None else 1)
        L = L if L is not None else (st.shape[1] if st is not None else 1)
        rc = lib.pr_seqmatch_create(None, cap, ch, None if st is None else st.ctypes.data_as(C.c_void_p), V, L, max_k, C.byref(h) if out else None)
        assert rc == _lib.PR_EINVAL and (not out or not h.value)
        return err()

    assert "out is NULL" in create(out=False)
    assert "steps is NULL" in create(steps=None)
    for cap in (0, -1, (1 << 24) + 1):
        assert "capacity=%d outside" % cap in create(cap=cap)
    for ch in (0, 3, 5, 8):
        assert "channels=%d is not 1, 2 or 4" % ch in create(ch=ch)
    assert "bad step table" in create(V=0) and "bad step table" in create(V=17, steps=np.zeros((17, 2)))
    assert "bad step table" in create(L=0) and "bad step table" in create(steps=np.zeros((1, 33)))
    assert "steps[v][0] != 0" in create(steps=[[0, 1], [1, 2]])
    assert "|steps[v][l]| > 64" in create(steps=[[0, 65]]) and "|steps[v][l]| > 64" in create(steps=[[0, 1], [0, -65]])
    for mk in (0, 129):
        assert "max_k=%d outside" % mk in create(max_k=mk)
    assert "ctx is NULL" in create()
    assert "handle is NULL" in (lib.pr_seqmatch_reset(None) == _lib.PR_EINVAL and err())
    a = C.addressof((C.c_double * 8)())
    assert lib.pr_seqmatch_push_dev(None, a, a, None, a, 1, 0, 1, a, a, a, a) == _lib.PR_EINVAL and "handle is NULL" in err()
    assert lib.pr_seqmatch_push(None, a, 0, a, 1, 0, 1, a, a, a, a) == _lib.PR_EINVAL
    assert lib.pr_seqmatch_read(None, None, None, None) == _lib.PR_EINVAL


def test_seq_steps_pinned():
    st = api.seq_steps(8, [1, -1, 0.75, -0.75, 0, 1.25])
    assert st.dtype == np.int32 and st.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7], [0, -1, -2, -3, -4, -5, -6, -7], [0, 1, 2, 2, 3, 4, 5, 5],
                                                    [0, -1, -2, -2, -3, -4, -5, -5], [0] * 8, [0, 1, 3, 4, 5, 6, 8, 9]]
    assert api.seq_steps(4, [0.5]).tolist() == [[0, 1, 1, 2]]                            # floor(|v| l + 0.5): halves round up ...
    assert api.seq_steps(4, [-0.5]).tolist() == [[0, -1, -1, -2]]                        # ... in magnitude, whatever the sign
    assert api.seq_steps(1, [1, -1, 3]).tolist() == [[0]]                                # identical rows are dropped
    assert api.seq_steps(3, [1, 1.1, -1, 0.9]).tolist() == [[0, 1, 2], [0, -1, -2]]      # ... keeping the first
    assert api.seq_steps(32, [2, -2]).shape == (2, 32) and api.seq_steps(32, [2])[0, 31] == 62
    for L, vel in ((4, [1, -1]), (8, [1, -1, 0.75, -0.75, 1.25, -1.25]), (5, [0, 0.3])):
        assert np.array_equal(api.seq_steps(L, vel), sq.seq_steps(L, vel))
    for bad in ((0, [1]), (33, [1]), (32, [2.2]), (4, []), (4, [float("nan")]), (2, list(np.linspace(1, 50, 17)))):
        with pytest.raises(ValueError):
            api.seq_steps(*bad)


def rand_case(seed, m, n, with_i=True):
    g = np.random.default_rng(seed)
    d_p = g.uniform(0.05, 1.0, (m, n)).astype(np.float32)
    d_i = g.uniform(0.05, 1.0, (m, n)).astype(np.float32) if with_i else None
    mom = np.stack([sq.row_moments(d_p), sq.row_moments(d_i)], 1) if with_i else None
    return d_p, d_i, mom


def test_single_lag_is_the_single_frame_selection():
    """L = 1, V = 1: the restatement is run_test.m's fusion, mask and top-k - the oracle's indices, its scores within 1e-9"""
    m, n, k, mw = 24, 97, 4, 5
    d_p, d_i, mom = rand_case(11, m, n)
    steps = np.zeros((1, 1), np.int32)
    idx, score, vel, S = sq.seq_select(d_p, d_i, mom, steps, 0, 0, mw, 2.0, k + 1)
    gaps = np.diff(score, axis=1)
    assert np.isfinite(score).all() and gaps.min() > 1e-6, gaps.min()                     # the top-(k + 1) is decided far above rounding
    oidx, osc = oracle_lib.fuse_topk(d_p.astype(np.float64), d_i.astype(np.float64), mw, 2.0, k)
    assert np.array_equal(idx[:, :k], oidx) and np.abs(score[:, :k] - osc).max() < 1e-9
    assert (vel == 0).all()


def triple_loop(d_p, d_i, mom, steps, q0, d0, mw, pw):
    """the rule cell by cell, in Python floats (IEEE doubles)"""
    m, n = d_p.shape
    V, L = steps.shape
    f = [[0.0] * n for _ in range(m)]
    for i in range(m):
        if d_i is not None:
            mp, sp = float(mom[i, 0, 1]), math.sqrt(float(mom[i, 0, 2]) / (float(mom[i, 0, 0]) - 1.0))
            mi, si = float(mom[i, 1, 1]), math.sqrt(float(mom[i, 1, 2]) / (float(mom[i, 1, 0]) - 1.0))
        for j in range(n):
            f[i][j] = float(d_p[i, j]) if d_i is None else pw * ((float(d_p[i, j]) - mp) / sp) + (float(d_i[i, j]) - mi) / si
    S = np.full((m, n), np.inf)
    vel = np.full((m, n), -1, np.int32)
    masked = lambda a, c: abs((q0 + a) - (d0 + c)) < mw
    for i in range(m):
        Li = min(L, i + 1)
        for j in range(n):
            if masked(i, j):
                continue
            for v in range(V):
                s, ok = 0.0, True
                for l in range(Li):
                    c = j - int(steps[v, l])
                    if not 0 <= c < n or masked(i - l, c) or math.isnan(f[i - l][c]):
                        ok = False
                        break
                    s += f[i - l][c]
                if not ok or math.isnan(s):
                    continue
                q = s / float(Li)
                if vel[i, j] < 0 or q < S[i, j]:
                    S[i, j], vel[i, j] = q, v
    return S, vel


@pytest.mark.parametrize("with_i", [True, False])
def test_dense_matrix_equals_the_triple_loop(with_i):
    for seed, m, n, steps, q0, d0, mw in ((1, 6, 9, [[0, 1, 2], [0, -1, -2], [0, 0, 0]], 0, 0, 0), (2, 7, 11, [[0, 1, 2, 3], [0, -2, -3, -5]], 3, 1, 2),
                                          (3, 3, 5, [[0, 1], [0, 1], [0, 4]], 0, 0, 1), (4, 5, 2, [[0, 0, 1]], 10, 12, 1)):
        d_p, d_i, mom = rand_case(seed, m, n, with_i)
        d_p[m // 2, n // 2] = np.nan
        d_p[0, 0] = np.inf
        st = np.array(steps, np.int32)
        S, vel = sq.seq_dense(d_p, d_i, mom, st, q0, d0, mw, 2.0)
        S2, vel2 = triple_loop(d_p, d_i, mom, st, q0, d0, mw, 2.0)
        assert np.array_equal(vel, vel2) and S.tobytes() == S2.tobytes(), (seed, with_i)


def test_row_offsets_change_only_the_indices():
    d_p, d_i, mom = rand_case(5, 20, 60)
    st = api.seq_steps(4, [1, -1, 0])
    a = sq.seq_select(d_p, d_i, mom, st, 0, 0, 3, 2.0, 5)
    b = sq.seq_select(d_p, d_i, mom, st, 1000, 1000, 3, 2.0, 5)
    assert np.array_equal(np.where(a[0] >= 0, a[0] + 1000, -1), b[0])
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    c = sq.seq_select(d_p, d_i, mom, st, 0, 77, 0, 2.0, 5)                               # without a mask the DB offset alone
    d = sq.seq_select(d_p, d_i, mom, st, 0, 0, 0, 2.0, 5)
    assert np.array_equal(c[0], d[0] + 77) and c[1].tobytes() == d[1].tobytes() and np.array_equal(c[2], d[2])


def alias_scene(seed, reverse, m=120, n=300):
    """A true cell at 0.6 among noise at 1.0 +- 0.1 in both channels; 30 % of the rows carry one alias at 0.35 (in both channels: a
    perceptual alias looks alike to both).  Forward: query i is DB row 90 + i; reverse: DB row 250 - i."""
    g = np.random.default_rng(seed)
    truth = (250 - np.arange(m)) if reverse else (90 + np.arange(m))
    d = [np.clip(g.normal(1.0, 0.1, (m, n)), 0.7, 1.3) for _ in range(2)]
    aliased = g.random(m) < 0.3
    alias = np.full(m, -1)
    for i in np.flatnonzero(aliased):
        while True:
            c = int(g.integers(0, n))
            if abs(c - truth[i]) > 20:
                break
        alias[i] = c
    for ch in d:
        ch[np.arange(m), truth] = 0.6
        ch[aliased, alias[aliased]] = 0.35
    d_p, d_i = d[0].astype(np.float32), d[1].astype(np.float32)
    return d_p, d_i, np.stack([sq.row_moments(d_p), sq.row_moments(d_i)], 1), truth, aliased


SCENE_L, SCENE_VEL = 8, [1, -1, 0.75, -0.75, 1.25, -1.25]


@pytest.mark.parametrize("seed,reverse", [(7, False), (8, False), (7, True), (8, True)])
def test_alias_scene(seed, reverse):
    d_p, d_i, mom, truth, aliased = alias_scene(seed, reverse)
    assert aliased.sum() >= 20
    single = sq.seq_select(d_p, d_i, mom, np.zeros((1, 1), np.int32), k=1)[0][:, 0]
    assert (single[aliased] != truth[aliased]).all() and (single[~aliased] == truth[~aliased]).all()
    idx, score, vel, _ = sq.seq_select(d_p, d_i, mom, api.seq_steps(SCENE_L, SCENE_VEL), k=2)
    late = np.arange(len(truth)) >= SCENE_L - 1
    assert (idx[late, 0] == truth[late]).all()
    gap = (score[late, 1] - score[late, 0]).min()
    print(f"alias scene seed {seed} reverse {reverse}: {int(aliased.sum())} aliased rows, smallest top-1 / top-2 gap {gap:.3f}")
    assert gap > 1.0, gap
    assert (vel[late, 0] == (1 if reverse else 0)).all()                                  # the unit velocity of the traversal's sign


def causal_rows(seed, N, cap, channels):
    """rows of a causal self-match: keyframe t sees distances to the t rows before it (the rest of the buffer is stale)"""
    g = np.random.default_rng(seed)
    return [np.where(np.arange(cap) < t, g.uniform(0.1, 1.0, (channels, cap)), g.uniform(5, 6, (channels, cap))) for t in range(N)]


def test_online_restatement_repeats_after_reset():
    cap, ch, N = 40, 2, 30
    rows = causal_rows(3, N, cap, ch)
    f = sq.SeqFilter(cap, ch, api.seq_steps(4, [1, -1, 0]), 4)
    run = lambda: [f.push(rows[t], t, (2.0, 1.0), True, 2, 3) for t in range(N)]
    a = run()
    ring_a, ids_a, pushes_a = f.ring.copy(), f.ids.copy(), f.pushes
    f.reset()
    assert f.pushes == 0 and not f.ring.any() and not f.ids.any()
    b = run()
    for x, y in zip(a, b):
        for u, w in zip(x, y):
            assert u.tobytes() == w.tobytes()
    assert ring_a.tobytes() == f.ring.tobytes() and np.array_equal(ids_a, f.ids) and pushes_a == f.pushes == N
    assert [int(x[3][1]) for x in a[:6]] == [1, 2, 3, 4, 4, 4]                            # L_n grows with the first L pushes
    assert (a[0][0] == -1).all() and (a[1][0] == -1).all()                                # n < 2: no candidate, still a push
    off = f.push(rows[5], 5, (2.0, 1.0), True, 2, 3, emitted=0)
    assert off[3].tolist() == [0, 0, N, 0] and (off[0] == -1).all() and ring_a.tobytes() == f.ring.tobytes() and f.pushes == N
    late = [x for x in a[12:]]
    assert all((x[0] >= 0).any() for x in late)
