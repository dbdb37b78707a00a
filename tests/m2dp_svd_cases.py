"""Clouds whose M2DP bin matrices have a leading singular pair that is tied, nearly tied, slow to separate or degenerate, pure numpy.

m2dp_svd_kernel is an iteration (8 squarings of the Gram matrix, then power steps on A A^T); what it does depends on s1 / s2 of the 64 x 128
matrix alone.  gen_edge_cases.py keeps every matrix at s1 / s2 >= 1.05; the cases here cover everything below.

Every cloud is about 200 points in tight clusters (sigma 1e-3 m) at one to three spots, on a hand-made identity frame
(pr_m2dp_generate_frames_dev), so the aligned points are known bit for bit.  All points of a cluster share one bin in every plane, so a plane's
row of the count matrix is n_A e_a + n_B e_b: A A^T is block diagonal over the groups of planes that share bins, and the singular values follow
from the group sizes g and the cluster sizes n.
  mirror : clusters of equal size at a and -a (intensities 9 and 1).  -a lands in the bin 8 sectors on, so both clusters group the planes
           alike: the count matrix has s_i = n sqrt(2 g_i), the intensity matrix (the bins of the brighter cluster) s_i = sqrt(g_i).  A spot
           with g_1 = g_2 ties BOTH channels of a row; g_1 / g_2 = 16/15 ... 11/10 gives 1.03 <= s1/s2 < 1.05, 25/24 ... 18/17 the grey band.
  two    : clusters of n_A and n_B points at unrelated spots; s1/s2 of the count matrix passes through 1 where n_A / n_B crosses the ratio
           of the two leading blocks, and the integers n_A, n_B around the crossing give 1.00007, 1.0007, 1.001, 1.004, 1.0075, 1.015, 1.025.
  far    : one cluster 1e4 m away.  Every plane drops it but the degenerate plane 32 (xProj = yProj = 0): one non-zero entry, s2 == 0.
  flat   : every intensity equal, so no bin mean exceeds the average: the all-zero intensity matrix (the kernel's fro == 0 branch).
The spots and sizes below were found by a seeded search with the oracle; `all_cases()` classifies what they give and
test_m2dp_svd_cases_cpu.py asserts the families and the guards, so a change of the oracle or of numpy cannot silently empty a family.

Bands of one matrix, from numpy.linalg.svd (LAPACK):  zero (s1 == 0), rank1 (s2 == 0), tie (s1 == s2 in double), near (1 < s1/s2 <= 1.01),
grey (1.01 < s1/s2 < 1.03), slow (1.03 <= s1/s2 < 1.05), well (>= 1.05).  The tied group of a matrix is its singular values >= s1 / 1.03.
"""
import numpy as np

import gen_edge_cases as G
import oracle_lib

MAX_RHO = G.MAX_RHO
SIGMA = 1e-3
NEAR_MAX, GREY_MAX, SLOW_MAX = 1.01, 1.03, 1.05
GROUP_RATIO = 1.03                  # the tied group: singular values >= s1 / 1.03
GAP_RATIO = 1.2                     # ... and the first value outside it is <= s1 / 1.2
UNRESOLVED = ("tie", "near", "grey")

# name, kind, spots, cluster sizes, intensities
SPECS = (
    ("tie_a", "mirror", [(-21.125, 19.178, 10.997)], [100, 100], [9, 1]),
    ("tie_b", "mirror", [(28.0, -2.515, 20.248)], [100, 100], [9, 1]),
    ("tie_c", "mirror", [(-20.263, 13.213, -6.332)], [100, 100], [9, 1]),
    ("tie3_a", "mirror", [(-24.119, 15.623, -7.95)], [100, 100], [9, 1]),
    ("tie3_b", "mirror", [(-10.411, -22.245, 27.135)], [100, 100], [9, 1]),
    ("near_00007", "two", [(16.337, -9.313, 25.394), (11.828, 2.253, 23.796)], [123, 68], [9, 1]),
    ("near_0007", "two", [(16.337, -9.313, 25.394), (11.828, 2.253, 23.796)], [130, 72], [9, 1]),
    ("near_001", "two", [(16.337, -9.313, 25.394), (11.828, 2.253, 23.796)], [118, 65], [9, 1]),
    ("near_004", "two", [(15.568, 2.391, -23.587), (21.971, -21.62, -3.621)], [67, 122], [9, 1]),
    ("near_0075", "two", [(15.568, 2.391, -23.587), (21.971, -21.62, -3.621)], [71, 114], [9, 1]),
    ("grey_015", "two", [(15.568, 2.391, -23.587), (21.971, -21.62, -3.621)], [60, 130], [9, 1]),
    ("grey_025", "two", [(15.568, 2.391, -23.587), (21.971, -21.62, -3.621)], [77, 105], [9, 1]),
    ("grey_027", "mirror", [(12.924, -0.541, 10.48)], [100, 100], [9, 1]),
    ("slow_a", "mirror", [(-29.994, -17.24, -12.618)], [100, 100], [9, 1]),
    # slow_tie, variant 3: a tie by construction in BOTH channels (g_1 = g_2).  LAPACK splits the count matrix (entries 100) by one ulp, so it
    # is classed "near" with s1/s2 = 1 + 2e-16 while the 0/1 intensity matrix is classed "tie"; the kernel treats both as exact ties
    ("slow_tie", "mirror", [(-9.745, -3.745, -12.143)], [100, 100], [9, 1]),
    ("flat", "mirror", [(-29.994, -17.24, -12.618)], [100, 100], [5, 5]),
    ("far", "far", [(6123.4, -5210.7, 5869.3)], [200], [7]),
    ("far_flat", "far", [(-5307.1, 6410.3, 5513.9)], [200], [4]),
)


def band_of(A):
    """(band, s1/s2, singular values) of one 64 x 128 matrix"""
    s = np.linalg.svd(A, compute_uv=False)
    if s[0] == 0:
        return "zero", np.inf, s
    if s[1] == 0:
        return "rank1", np.inf, s
    r = s[0] / s[1]
    return ("tie" if r == 1 else "near" if r <= NEAR_MAX else "grey" if r < GREY_MAX else "slow" if r < SLOW_MAX else "well"), r, s


def tied_group(s):
    """number of singular values in the tied group"""
    return int((s >= s[0] / GROUP_RATIO).sum())


def gap_ok(s):
    """the first singular value outside the tied group is at most s1 / 1.2"""
    k = tied_group(s)
    return k == len(s) or s[k] <= s[0] / GAP_RATIO


def _clusters(spots, sizes, intens, seed):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.asarray(sp, np.float64)[None] + rng.normal(0.0, SIGMA, (n, 3)) for sp, n in zip(spots, sizes)])
    it = np.concatenate([np.full(n, v, np.float32) for n, v in zip(sizes, intens)])
    p = rng.permutation(len(pts))              # the clusters interleaved: both reach every wave of the binning kernel
    return pts[p], it[p]


class SvdCase:
    """name, kind, xyz [P,3], inten [P] float32, frame [16], aligned [P,3], offs, max_rho; rows [4,384]: the oracle's signature rows; mats
    [4,2,64,128]; band[v][ch], ratio[v][ch], sv[v][ch]: the band, s1/s2 and singular values of matrix (variant, channel)"""

    def __init__(self, name, kind, spots, sizes, intens, index):
        self.name, self.kind, self.max_rho = name, kind, MAX_RHO
        spots = [np.asarray(s, np.float64) for s in spots]
        if kind == "mirror":
            spots = [spots[0], -spots[0]]
        for attempt in range(16):              # the first seed whose points all keep the guard distance from every bin edge
            xyz, inten = _clusters(spots, sizes, intens, 1000 * index + attempt)
            if G.m2dp_guard(xyz, MAX_RHO).min() > G.GUARD_BINS:
                break
        else:
            raise AssertionError(f"{name}: no draw keeps the guard distance")
        self.xyz, self.inten = xyz, inten
        self.frame = G.make_frame("identity", len(xyz), inten)
        self.aligned = G.align(self.frame, xyz)
        self.offs = np.array([0, len(xyz)], np.int64)
        self.rows, self.mats = oracle_lib.m2dp_signature_aligned(self.aligned, inten, MAX_RHO, with_matrices=True)
        cls = [[band_of(self.mats[v, ch]) for ch in range(2)] for v in range(4)]
        self.band = [[c[0] for c in r] for r in cls]
        self.ratio = [[c[1] for c in r] for r in cls]
        self.sv = [[c[2] for c in r] for r in cls]

    def row_class(self, v):
        """'truth': a matrix of the row at s1/s2 <= 1.01 (always named); 'grey': one in the grey band and none below (may be named);
        'clean': every matrix at s1/s2 >= 1.03, rank 1 or zero (never named)"""
        b = self.band[v]
        return "truth" if ("tie" in b or "near" in b) else "grey" if "grey" in b else "clean"


_CACHE = []


def all_cases():
    """the list of cases, built once per process"""
    if not _CACHE:
        _CACHE.extend(SvdCase(nm, kind, spots, sizes, intens, i) for i, (nm, kind, spots, sizes, intens) in enumerate(SPECS))
    return _CACHE


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


def clean_cases():
    """the cases none of whose rows can be named"""
    return [c for c in all_cases() if all(c.row_class(v) == "clean" for v in range(4))]


def expected_rows(batch):
    """(truth, grey): the sets of signature rows cloud * 4 + variant of a batch (a list of cases) that are always / possibly named"""
    truth, grey = set(), set()
    for i, c in enumerate(batch):
        for v in range(4):
            k = c.row_class(v)
            if k == "truth":
                truth.add(4 * i + v)
            elif k == "grey":
                grey.add(4 * i + v)
    return truth, grey
