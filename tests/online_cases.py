"""The committed match cases of the online signature database (test_online_cpu.py checks their separation on the oracle,
test_gpu_online.py runs them on the device): per descriptor type ONE database of 1025 synthetic signatures and one query, matched
while the database holds its first n rows, n at the kernels' edges; and a small SC database with the reference's corner rules."""
import functools
import os
import re

import numpy as np

import online_model
from so_dso_place_recognition_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_blocks():
    """ONLINE_NB of the source: the most workgroups of the rows kernel (entry j belongs to workgroup j % NB)"""
    txt = open(os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc", "online.hpp")).read()
    return int(re.search(r"constexpr int ONLINE_NB = (\d+);", txt).group(1))


NB = rows_blocks()
COUNTS = tuple(sorted({0, 1, 2, 3, NB - 1, NB, NB + 1, 255, 256, 257, 1023, 1024, 1025}))
NMAX = 1025
MASK_ALL = 2000                                        # above every count: every entry is masked
# (k, mask_width): k in {1, 5} x every mask, and k = 7 - above the counts 0 .. 3, like 5
KM = tuple((k, w) for k in (1, 5) for w in (0, 1, 10, MASK_ALL)) + ((7, 0), (7, 10))
MAX_K = 8
SEEDS = {"sc": 910, "m2dp": 920}


@functools.lru_cache(maxsize=None)
def edge_case(type_):
    """dict(db [NMAX * rps, L], q [rps, L], dp / di [NMAX]: the oracle's distances of q to every row)"""
    seed = SEEDS[type_]
    if type_ == "sc":
        db = synth.sc_database(seed, NMAX)
        q, _ = synth.sc_queries(seed + 1, db[:3], 1)
    else:
        db = synth.m2dp_database(seed, NMAX)
        q, _ = synth.m2dp_queries(seed + 1, db[:12], 1)
    dp, di = online_model.distances(type_, q, db)
    for a in (db, q, dp, di):
        a.setflags(write=False)
    return dict(db=db, q=q, dp=dp, di=di)


@functools.lru_cache(maxsize=None)
def corner_case():
    """40 SC rows: row 5 all zero (zero norm: NaN distances), row 20 an exact copy of row 7 and row 33 of row 12; queries: planted on
    row 7 (its two copies tie), and all zero."""
    db = synth.sc_database(930, 40)
    db[5] = 0.0
    db[20] = db[7]
    db[33] = db[12]
    q, _ = synth.sc_queries(931, db[7:8], 1)
    db.setflags(write=False); q.setflags(write=False)
    return dict(db=db, q=q, zero=np.zeros((1, 2400)), copies=((7, 20), (12, 33)), zero_row=5)


CORNER_COUNTS = (6, 21, 40)                            # the zero row alone, + the first pair of copies, everything
CORNER_KM = ((1, 0), (5, 0), (5, 3))
CORNER_WEIGHTS = (1.0, 2.0)


def same_rows(db, rps, a, b):
    return db[a * rps:(a + 1) * rps].tobytes() == db[b * rps:(b + 1) * rps].tobytes()


def separated(db, rps, idx, score, tol=1e-6):
    """The condition under which a device result must equal the oracle's index for index: consecutive scores of the list differ by more
    than tol or belong to rows that are exact copies (identical distances by construction, so the index decides on both sides).  Two
    +Inf scores - both rows under the mask, equal by rule and not by arithmetic - are ordered by index alone as well."""
    for t in range(len(idx) - 1):
        a, b = int(idx[t]), int(idx[t + 1])
        if a < 0 or b < 0:
            break
        sa, sb = float(score[t]), float(score[t + 1])
        if np.isinf(sa) and np.isinf(sb):
            continue
        if not (sb - sa > tol or same_rows(db, rps, a, b)):
            return False
    return True
