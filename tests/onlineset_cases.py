"""The committed match cases of the online signature sets (test_onlineset_cpu.py checks their separation on the oracle,
test_gpu_onlineset.py runs them on the device): per kind ONE database of 1025 synthetic keyframes and one query planted on row 1,
matched while the set holds its first n rows, n at the kernels' edges; and small databases with the reference's corner rules."""
import functools
import os
import re

import numpy as np

import online_cases
import onlineset_model
from so_dso_place_recognition_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_constants():
    """(ONLINESET_NB_FUSED, ONLINESET_NB_DELIGHT) of the source: the most workgroups of the two rows kernels (fused: entry j belongs to
    workgroup j % NB; DELIGHT: batch j // 16 to workgroup (j // 16) % NB)"""
    txt = open(os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc", "onlineset.hpp")).read()
    return tuple(int(re.search(r"constexpr int ONLINESET_NB_%s = (\d+);" % n, txt).group(1)) for n in ("FUSED", "DELIGHT"))


NB_FUSED, NB_DELIGHT = grid_constants()
NMAX = 1025
KM = online_cases.KM
MAX_K = online_cases.MAX_K
WEIGHTS = (1.0, 2.0)
FUSED_COUNTS = online_cases.COUNTS                     # 0 .. 3, NB - 1 .. NB + 1, 255 .. 257, 1023 .. 1025 (NB = ONLINE_NB = ONLINESET_NB_FUSED)
DELIGHT_BATCH = 16                                     # exact_batch's pairs per workgroup and stride
DELIGHT_EDGE = DELIGHT_BATCH * NB_DELIGHT              # the first row that a workgroup's SECOND stride takes
DELIGHT_COUNTS = tuple(sorted({0, 1, 2, 15, 16, 17, DELIGHT_EDGE - 1, DELIGHT_EDGE, DELIGHT_EDGE + 1}))
RPS = {"sc": 1, "m2dp": 4, "delight": 16}


def rows_of(kind, db, n0, n1=None):
    """the parts' rows of entries [n0, n1) (n1 None: the one entry n0) of db = the tuple of the parts' arrays"""
    n1 = n0 + 1 if n1 is None else n1
    return tuple(a[n0 * r:n1 * r] for a, (_, r, _) in zip(db, onlineset_model.PARTS[kind]))


@functools.lru_cache(maxsize=None)
def fused_edge_case():
    """dict(db (sc [NMAX, 2400], m2dp [4 NMAX, 384]), q (sc [1, 2400], m2dp [4, 384]) planted on row 1 of both, d [4, NMAX])"""
    sc = synth.sc_database(910, NMAX)
    m2 = synth.m2dp_database(920, NMAX)
    qs, _ = synth.sc_queries(911, sc[1:2], 1)
    qm, _ = synth.m2dp_queries(921, m2[4:8], 1)
    d = onlineset_model.distances("fused", (qs, qm), (sc, m2))
    for a in (sc, m2, qs, qm, d):
        a.setflags(write=False)
    return dict(db=(sc, m2), q=(qs, qm), d=d)


@functools.lru_cache(maxsize=None)
def fused_corner_case():
    """40 keyframes.  SC: row 5 all zero (NaN distances), row 20 = row 7, row 33 = row 12.  M2DP: entry 20 = entry 7 only - so 7 and 20
    are copies in EVERY part (they tie), 12 and 33 are not.  Queries: planted on row 7 of both parts, and one with an all-zero SC part."""
    sc = synth.sc_database(930, 40)
    sc[5] = 0.0
    sc[20] = sc[7]
    sc[33] = sc[12]
    m2 = synth.m2dp_database(935, 40)
    m2[80:84] = m2[28:32]
    qs, _ = synth.sc_queries(931, sc[7:8], 1)
    qm, _ = synth.m2dp_queries(936, m2[28:32], 1)
    for a in (sc, m2, qs, qm):
        a.setflags(write=False)
    return dict(db=(sc, m2), q=(qs, qm), zero=(np.zeros((1, 2400)), qm), copies=((7, 20),), sc_only_copies=((12, 33),), zero_row=5)


@functools.lru_cache(maxsize=None)
def delight_edge_case():
    """dict(db ([16 NMAX, 256],), q ([16, 256],) planted on row 1, d [1, NMAX])"""
    db = synth.delight_database(940, NMAX)
    q, _ = synth.delight_queries(941, db[16:32], 1)
    d = onlineset_model.distances("delight", q, (db,))
    for a in (db, q, d):
        a.setflags(write=False)
    return dict(db=(db,), q=(q,), d=d)


@functools.lru_cache(maxsize=None)
def delight_corner_case():
    """40 entries: entry 5 all zero, entry 20 = entry 7; queries: planted on entry 7, and all zero (zero against zero: no bin with
    A + B > 0, 0 / 0 = NaN fails `best > ts`, so the distance is +Inf - last, but selectable)."""
    db = synth.delight_database(950, 40)
    db[5 * 16:6 * 16] = 0.0
    db[20 * 16:21 * 16] = db[7 * 16:8 * 16]
    q, _ = synth.delight_queries(951, db[7 * 16:8 * 16], 1)
    db.setflags(write=False); q.setflags(write=False)
    return dict(db=(db,), q=(q,), zero=(np.zeros((16, 256)),), copies=((7, 20),), zero_row=5)


CORNER_COUNTS = online_cases.CORNER_COUNTS             # 6, 21, 40
CORNER_KM = online_cases.CORNER_KM
CORNER_WEIGHTS = online_cases.CORNER_WEIGHTS


def same_rows(kind, db, a, b):
    """copies only if EVERY part is a copy"""
    return all(x.tobytes() == y.tobytes() for x, y in zip(rows_of(kind, db, a), rows_of(kind, db, b)))


def separated(kind, db, idx, score, tol=1e-6):
    """online_cases.separated for a set: consecutive scores of the list differ by more than tol, or belong to rows that are exact copies
    in every part (identical distances by construction, so the index decides on both sides), or are both +Inf (equal by rule)."""
    for t in range(len(idx) - 1):
        a, b = int(idx[t]), int(idx[t + 1])
        if a < 0 or b < 0:
            break
        sa, sb = float(score[t]), float(score[t + 1])
        if np.isinf(sa) and np.isinf(sb):
            continue
        if not (sb - sa > tol or same_rows(kind, db, a, b)):
            return False
    return True
