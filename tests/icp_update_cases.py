"""The committed, seeded cases of the ICP UPDATE tests (test_icp_update_cpu.py, test_gpu_icp_update.py): one Kabsch step of
csrc/icp.hip's icp_finish_kernel against the 60-digit reference icp_mp.py, where icp_cases.py's six fat, centred, small-yaw scenes cannot
see it go wrong.  A case is (P, Q, T0, max_corr, min_inliers); the pairs of a case are whatever icp_np.nn finds under T0 (nothing is
planted: the Kabsch optimum of any pair set is well defined), and test_icp_update_cpu.py proves the 1e-9 margins that make the device
choose the same ones.

  cond_*      conditioning: inlier sets whose H has s2 / s1 of about 1, 1e-2, ... 1e-10 - needles (s2 ~ s3) and planks (s3 << s2 << s1), 300
              points, 20 m long, lying obliquely in space; Q is a rigid motion of P, each with jitter of 0.2 % of the thin extent (2 cm on
              10 m); T0 is the motion turned by 3 or by 25 degrees about an oblique axis
  degen_*     the degeneracy rule s2 <= 1e-12 s1: an exact line, that line with 1e-15-relative dust, a needle 10 x below the threshold and
              one 10 x above it, each at the origin and 45 m and 100 m away (the exact line also 1e3 and 1e4 m away)
  motion_*    a fat lattice cloud with exact pairs: total motions of 90 degrees about x and z, 180 and 179.999 degrees (the update
              itself is the seed's 2 degrees), an update of 1e-7 degrees from the identity seed; the eight corners of a cube (H an exact multiple of a rotation: s1 = s2 = s3) and a square (s1 = s2, s3 = 0)
  reflect_*   near-planar sets whose out-of-plane jitter is mirrored between P and Q: the unconstrained optimum is a reflection, d = -1
  pos_*       the fat cloud 0, 45, 100, 1e3 and 1e4 m along (1, 1, 1) and along y; a target whose first row is NaN, has an infinite
              coordinate or is a finite point 1e6 m or 1e200 away (nobody's correspondence: the sums must not feel it), an empty target
  red_*       source sizes around the chunk sizes (256 and 1024 points) with all points, every second point, all but one whole middle
              chunk, or three points (the last of the last chunk among them) as inliers; n_inl = min_inliers and min_inliers - 1
  full_*      whole refinements: a needle (s2 / s1 about 1e-5) and a plank whose Q is an exact rigid motion of P

The bound: tol_R = 32 eps s1 / s2 + 1e-13 on the entries of R - the linear term is what a
backward-stable solve of H guarantees, the factor and the floor cover the order of the sums - and tol_t = tol_R (1 + |mu_p'|) +
1e-12 (1 + |mu_q|) metres, s1, s2 and the means from the reference."""
import functools

import numpy as np

import icp_mp
import icp_np

EPS = 2.0 ** -52
AXIS = (0.3, -0.8, 0.5)
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])
UPDATE, DEGENERATE, TOO_FEW = "update", "degenerate", "too_few"


def rot(deg, axis=AXIS):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rigid(deg, t, axis=AXIS):
    return np.hstack([rot(deg, axis), np.asarray(t, np.float64).reshape(3, 1)])


def compose(A, B):
    """x -> A(B(x)) for [3, 4] motions."""
    return np.hstack([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]])


def moved(P, M):
    return P @ M[:, :3].T + M[:, 3]


def shifted(P, Q, T0, c):
    """The same scene seen from an origin c metres away: P + c, Q + c and the seed that maps one onto the other as T0 did."""
    c = np.asarray(c, np.float64)
    return P + c, Q + c, np.hstack([T0[:, :3], (T0[:, 3] + c - T0[:, :3] @ c)[:, None]])


LIE = rot(33.0, (0.5, 0.4, -0.77))            # how the long clouds lie in space: no extent along a coordinate axis
MOTION = rigid(40.0, (0.3, 0.02, -0.2), (0.2, 0.5, -0.7))


def _slab(seed, n, ext, jitter, off_deg, exact=False):
    """n points uniform in a box of the extents ext, lying obliquely (LIE); Q = MOTION(P); jitter on both; T0 = MOTION turned by off_deg."""
    rng = np.random.default_rng(seed)
    base = (rng.random((n, 3)) - 0.5) * np.asarray(ext, np.float64)
    base = base @ LIE.T
    P = base + (0 if exact else rng.normal(0, jitter, base.shape))
    Q = moved(base, MOTION) + (0 if exact else rng.normal(0, jitter, base.shape))
    T0 = compose(rigid(off_deg, (0.01, -0.02, 0.015)), MOTION)
    return P, Q, T0


WIDEN = {("needle", 0): 1.0, ("needle", 2): 1.0, ("needle", 4): 1.6, ("needle", 6): 3.0, ("needle", 8): 3.0, ("needle", 10): 3.0,
         ("plank", 2): 1.0, ("plank", 4): 3.7, ("plank", 6): 3.0, ("plank", 8): 3.0, ("plank", 10): 4.0}


def _cond(k, shape, off_deg, seed):
    w = 20.0 * 10.0 ** (-k / 2.0)                                   # s2 / s1 ~ (w / L)^2 = 10^-k
    if off_deg > 10:
        w *= WIDEN[shape, k]                                                # so far off, the pairs scramble the thin directions of a thin cloud
    ext = (20.0, w, w) if shape == "needle" else (20.0, w, w * 1e-2)
    P, Q, T0 = _slab(seed, 300, ext, 2e-3 * ext[2], off_deg)
    return dict(P=P, Q=Q, T0=T0, max_corr=50.0, min_inliers=3, expect=UPDATE, band=(10.0 ** (-k - 0.8), min(1.0, 10.0 ** (-k + 0.3))), d=1)


def _lattice(seed, side=5, pitch=2.0, wobble=0.25):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side) - (side - 1) / 2.0] * 3, indexing="ij"), -1).reshape(-1, 3) * pitch
    return g + rng.uniform(-wobble, wobble, g.shape)


def _fat(seed, motion=MOTION, off_deg=2.0, max_corr=1.0):
    """A fat cloud of 125 well-separated points (2 m pitch) seen twice with 2 cm jitter; the seed is 2 degrees and 3 cm off the motion."""
    rng = np.random.default_rng(seed)
    base = _lattice(seed)
    P = base + rng.normal(0, 0.02, base.shape)
    Q = moved(base, motion) + rng.normal(0, 0.02, base.shape)
    T0 = compose(rigid(off_deg, (0.01, -0.02, 0.015)), motion)
    return dict(P=P, Q=Q, T0=T0, max_corr=max_corr, min_inliers=3, expect=UPDATE, band=(0.2, 1.0), d=1)


def _exact_pairs(seed, motion, off):
    """The lattice and its image under `motion`, no jitter; the seed is `off` (a motion) after `motion`."""
    base = _lattice(seed)
    return dict(P=base, Q=moved(base, motion), T0=compose(off, motion), max_corr=1.0, min_inliers=3, expect=UPDATE, band=(0.2, 1.0), d=1)


def _tiny_update(seed, deg):
    """The lattice and its image under a rotation of `deg` degrees about AXIS; the seed is the IDENTITY, so the update itself is that
    rotation (off-diagonal entries of dR of about 1.7e-9 for 1e-7 degrees) and has to come out within the bound's 1e-13."""
    base = _lattice(seed)
    return dict(P=base, Q=moved(base, rigid(deg, (0.0, 0.0, 0.0))), T0=IDENT.copy(), max_corr=1.0, min_inliers=3, expect=UPDATE, band=(0.2, 1.0), d=1,
                update_deg=deg)


def _degen(kind, offset):
    """20 points along (3, 5, -7) / 4 steps: an exact line in fp64; dust and needles add a perpendicular spread of the stated relative
    size.  Source = target + a 1 cm step along the line (correspondences i -> i), seed = identity."""
    rng = np.random.default_rng({"line": 71, "dust": 72, "below": 73, "above": 74}[kind])
    u = np.array([3.0, 5.0, -7.0]) / 4.0
    a = np.arange(20.0) - 8.0
    Q = np.outer(a, u)
    length = 19.0 * np.linalg.norm(u)
    rel = {"line": 0.0, "dust": 1e-15, "below": 2.5e-7, "above": 1.2e-5}[kind]      # s2 / s1 ~ 4 rel^2 of a uniform spread
    Q = Q + (rng.random(Q.shape) - 0.5) * (rel * length)
    P = Q + u * (0.01 / np.linalg.norm(u)) + (rng.random(Q.shape) - 0.5) * (rel * length)
    c = offset * np.array([0.6, -0.64, 0.48])
    if kind == "line":
        c = np.round(c * 4.0) / 4.0                                  # keeps the line exact in fp64
    P, Q, T0 = shifted(P, Q, IDENT, c)
    band = {"line": (0.0, 1e-40), "dust": (0.0, 1e-13), "below": (1e-15, 1e-13), "above": (1e-11, 1e-9)}[kind]
    return dict(P=P, Q=Q, T0=T0, max_corr=1.0, min_inliers=3, expect=UPDATE if kind == "above" else DEGENERATE, band=band, d=1)


def _cube(square):
    c = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    if square:
        c = c[c[:, 2] > 0] * [1.0, 1.0, 0.0]
    T0 = rigid(30.0, (0.0, 0.0, 0.0))                                # p' = R0 c, q = c: H = R0 sum c c^T, a multiple of R0 for the cube
    return dict(P=c, Q=c.copy(), T0=T0, max_corr=2.0, min_inliers=3, expect=UPDATE, band=(0.999999, 1.0), d=1)


def _reflect(seed, off_deg):
    """A 9 x 9 grid of 1 m pitch in a tilted plane; the out-of-plane jitter (5 cm) of Q is the mirror image of P's."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(9) - 4.0, np.arange(9) - 4.0, indexing="ij"), -1).reshape(-1, 2)
    g = g + rng.uniform(-0.1, 0.1, g.shape)
    z = rng.normal(0, 0.05, len(g))
    tilt = rot(28.0, (0.9, -0.1, 0.4))
    P = np.column_stack([g, z]) @ tilt.T
    Q = moved(np.column_stack([g, -z]) @ tilt.T, MOTION)
    T0 = compose(rigid(off_deg, (0.01, -0.02, 0.015)), MOTION)
    return dict(P=P, Q=Q, T0=T0, max_corr=1.0, min_inliers=3, expect=UPDATE, band=(0.3, 1.0), d=-1)


def _pos(offset, direction):
    c = _fat(31)
    c["P"], c["Q"], c["T0"] = shifted(c["P"], c["Q"], c["T0"], offset * np.asarray(direction, np.float64))
    return c


def _odd_target(kind):
    """What the pivot of the device's sums must not depend on: a target whose first row is NaN, has an infinite coordinate, or is a finite
    but wild point (a max-range sentinel 1e6 m away, 1e200) - nobody's correspondence in each case -, and an empty target (no inliers)."""
    c = _fat(33)
    if kind == "empty":
        c["Q"] = np.zeros((0, 3))
        c["expect"] = TOO_FEW
    else:
        first = {"nan": [np.nan] * 3, "inf": [1.0, np.inf, -2.0], "1e6": [1e6, -1e6, 1e6], "1e200": [1e200, 0.0, -1e200]}[kind]
        c["P"], c["Q"], c["T0"] = shifted(c["P"], c["Q"], c["T0"], (30.0, -20.0, 10.0))
        c["Q"] = np.vstack([first, c["Q"]])
    return c


RED_SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 513, 1023, 1024, 1025)
RED_PATTERNS = ("all", "second", "midchunk", "three")


def _red_inliers(n, pattern):
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "second":
        keep[::2] = True
    elif pattern == "midchunk":                                      # a whole chunk of 256 outliers, with inliers in front of it and behind it
        keep[:] = True
        keep[256:512] = False
    else:                                                            # the last point of the last chunk and two others
        keep[[0, n // 2, n - 1]] = True
    return keep


def _red(n, pattern, seed, min_inliers=3, inliers=None):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    base = (g[rng.permutation(len(g))[:n]] - (side - 1) / 2.0) * 2.0 + rng.uniform(-0.25, 0.25, (n, 3))
    keep = _red_inliers(n, pattern) if inliers is None else np.arange(n) < inliers
    P = base + rng.normal(0, 0.02, base.shape)
    P[~keep] += [0.0, 0.0, 10.0 + 2.0 * side]                        # the outliers: 10 m above the target's top
    Q = moved(base, MOTION) + rng.normal(0, 0.02, base.shape)
    T0 = compose(rigid(1.0, (0.01, -0.02, 0.015)), MOTION)
    n_inl = int(keep.sum())
    return dict(P=P, Q=Q, T0=T0, max_corr=1.0, min_inliers=min_inliers, expect=UPDATE if n_inl >= min_inliers else TOO_FEW, band=(1e-3, 1.0),
                d=1, n_inl=n_inl)


def _full(shape):
    ext = (10.0, 10.0 * 10.0 ** -2.5, 10.0 * 10.0 ** -2.5) if shape == "needle" else (10.0, 1.0, 0.01)
    P, Q, T0 = _slab(91 if shape == "needle" else 92, 300, ext, 0.0, 1.0, exact=True)
    T0 = compose(rigid(0.02, (0.001, -0.002, 0.0015)), MOTION)
    return dict(P=P, Q=Q, T0=T0, max_corr=1.0, min_inliers=3, expect=UPDATE, band=(10.0 ** -6.5, 10.0 ** -3.5) if shape == "needle" else (1e-4, 1e-1), d=1)


BUILDERS = {}
for _k in (0, 2, 4, 6, 8, 10):
    for _shape in (("fat",) if _k == 0 else ("needle", "plank")):
        for _deg in (3, 25):
            BUILDERS["cond_%s_1e-%d_%ddeg" % (_shape, _k, _deg)] = functools.partial(_cond, _k, "needle" if _shape == "fat" else _shape, _deg,
                                                                                     100 + 10 * _k + _deg + (1 if _shape == "plank" else 0))
for _kind in ("line", "dust", "below", "above"):
    for _off in (0, 45, 100) + ((1000, 10000) if _kind == "line" else ()):            # the far exact lines: what pivoted sums are for
        BUILDERS["degen_%s_%dm" % (_kind, _off)] = functools.partial(_degen, _kind, float(_off))
BUILDERS["motion_x90"] = functools.partial(_exact_pairs, 41, rigid(90.0, (0.5, -0.3, 0.2), (1, 0, 0)), rigid(2.0, (0.01, -0.02, 0.015)))
BUILDERS["motion_z90"] = functools.partial(_exact_pairs, 42, rigid(90.0, (0.5, -0.3, 0.2), (0, 0, 1)), rigid(2.0, (0.01, -0.02, 0.015)))
BUILDERS["motion_180"] = functools.partial(_exact_pairs, 43, rigid(180.0, (0.5, -0.3, 0.2)), rigid(2.0, (0.01, -0.02, 0.015)))
BUILDERS["motion_179.999"] = functools.partial(_exact_pairs, 44, rigid(179.999, (0.5, -0.3, 0.2)), rigid(2.0, (0.01, -0.02, 0.015)))
BUILDERS["motion_1e-7deg"] = functools.partial(_tiny_update, 45, 1e-7)
BUILDERS["motion_cube8"] = functools.partial(_cube, False)
BUILDERS["motion_square"] = functools.partial(_cube, True)
BUILDERS["reflect_3deg"] = functools.partial(_reflect, 51, 3.0)
BUILDERS["reflect_1deg"] = functools.partial(_reflect, 52, 1.0)
for _off in (0, 45, 100, 1000, 10000):
    BUILDERS["pos_111_%dm" % _off] = functools.partial(_pos, float(_off), (1, 1, 1))
    if _off:
        BUILDERS["pos_y_%dm" % _off] = functools.partial(_pos, float(_off), (0, 1, 0))
for _kind in ("nan", "inf", "1e6", "1e200", "empty"):
    BUILDERS["pos_first_target_%s" % _kind] = functools.partial(_odd_target, _kind)
for _n in RED_SIZES:
    for _pat in RED_PATTERNS:
        if _pat == "midchunk" and _n < 513:
            continue                                                 # needs points behind the second chunk
        BUILDERS["red_%d_%s" % (_n, _pat)] = functools.partial(_red, _n, _pat, 600 + _n)
BUILDERS["red_65_at_min_inliers"] = functools.partial(_red, 65, None, 701, 7, 7)
BUILDERS["red_65_below_min_inliers"] = functools.partial(_red, 65, None, 702, 7, 6)

CASES = tuple(BUILDERS)
COND = tuple(n for n in CASES if n.startswith("cond_"))
RED = tuple(n for n in CASES if n.startswith("red_"))
FAR = tuple(n for n in CASES if n.startswith("pos_") and n.endswith(("_1000m", "_10000m")))
FULL = {"full_needle": functools.partial(_full, "needle"), "full_plank": functools.partial(_full, "plank")}
MANY = "red_1025_all"                                                # the cloud pair 4100 pairs share (the four-points-per-lane kernel)


@functools.lru_cache(maxsize=None)
def case(name):
    c = (BUILDERS.get(name) or FULL[name])()
    for k in ("P", "Q", "T0"):
        c[k] = np.ascontiguousarray(c[k], np.float64)
        c[k].setflags(write=False)
    assert len(c["P"]) <= 1025 and len(c["Q"]) <= 1025
    return c


@functools.lru_cache(maxsize=None)
def pairs(name):
    """The case's correspondences under T0 as the restatement finds them: dict(idx, d2, inl, p, q, nn_margin, corr_margin)."""
    c = case(name)
    Pt = icp_np.transform(c["T0"], c["P"])
    idx, d2, gap = icp_np.nn(Pt, c["Q"], margins=True)
    mc2 = c["max_corr"] * c["max_corr"]
    fin = d2[d2 < np.inf]
    inl = d2 < mc2
    return dict(idx=idx, d2=d2, inl=inl, p=Pt[inl], q=c["Q"][idx[inl]], nn_margin=gap,
                corr_margin=float((np.abs(fin - mc2) / mc2).min()) if len(fin) else np.inf)


@functools.lru_cache(maxsize=None)
def reference(name):
    """icp_mp's update of the case's pairs (computed once per process, shared by the tests, never modified); None without inliers."""
    pr = pairs(name)
    return icp_mp.kabsch_update(pr["p"], pr["q"], case(name)["T0"]) if len(pr["p"]) else None


@functools.lru_cache(maxsize=None)
def restatement(name, order="pairwise"):
    """icp_np's one step: max_iter = 1 and both tolerances 0."""
    c = case(name)
    return icp_np.icp(c["P"], c["Q"], c["T0"], max_iter=1, max_corr=c["max_corr"], tol_rmse=0.0, tol_fitness=0.0, min_inliers=c["min_inliers"],
                      order=order)


def bound(ref):
    """(tol_R, tol_t) of a reference update."""
    tol_R = 32.0 * EPS * ref["s"][0] / ref["s"][1] + 1e-13
    return tol_R, tol_R * (1.0 + np.linalg.norm(ref["mu_p"])) + 1e-12 * (1.0 + np.linalg.norm(ref["mu_q"]))


def error(T, ref):
    """(max |dR|, max |dt|) of T against the reference's T."""
    d = np.abs(np.asarray(T, np.float64).reshape(3, 4) - ref["T"])
    return float(d[:, :3].max()), float(d[:, 3].max())


def over(T, ref):
    """The larger of the two errors of T as a multiple of its bound."""
    (eR, et), (tR, tt) = error(T, ref), bound(ref)
    return max(eR / tR, et / tt)
