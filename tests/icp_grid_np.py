"""The uniform-grid correspondence search of the ICP stage (csrc/icp_grid.hip) restated in NumPy.  Its normative result
is icp_np.py's with the correspondences masked to d2 < max_corr^2: `nn_radius` is what pr_icp_nn_radius returns in either search mode,
`icp_masked` is icp_np.icp run on masked correspondences - bit for bit the unmasked run (test_icp_grid_cpu.py), because only inliers
enter an update or a statistic.  `cell_edge` / `cell_coord` restate the two formulas of the grid as the source states them (the test pins
them to the source text); the containment argument is about them."""
import numpy as np

import icp_np

SLACK = 1.0 + 2.0 ** -10          # ICP_GRID_SLACK: h >= max_corr * SLACK
COORD_BOUND = 2.0 ** 1000         # the containment argument holds for coordinates and max_corr up to this magnitude


def mask(idx, d2, max_corr):
    keep = d2 < max_corr * max_corr
    return np.where(keep, idx, -1).astype(np.int32), np.where(keep, d2, np.inf)


def nn_radius(Pt, Q, max_corr):
    """(idx, d2): the first-minimum nearest neighbour where its d2 < max_corr^2, (-1, +Inf) elsewhere."""
    idx, d2 = icp_np.nn(Pt, Q)
    return mask(idx, d2, max_corr)


def icp_masked(P, Q, T0, max_corr=1.0, **kw):
    """icp_np.icp with every correspondence pass masked to the radius (the margins then describe the masked passes)."""
    plain = icp_np.nn

    def masked(Pt, Q_, margins=False, block=512):
        idx, d2, gap = plain(Pt, Q_, margins=True, block=block)
        idx, d2 = mask(idx, d2, max_corr)
        return (idx, d2, gap) if margins else (idx, d2)

    icp_np.nn = masked
    try:
        return icp_np.icp(P, Q, T0, max_corr=max_corr, **kw)
    finally:
        icp_np.nn = plain


def cell_edge(max_corr, ext, G):
    """fmax(max_corr * ICP_GRID_SLACK, ext / (double)G)"""
    with np.errstate(over="ignore"):
        return np.maximum(np.float64(max_corr) * SLACK, np.float64(ext) / np.float64(G))


def cell_coord(x, x0, h):
    """floor((x - x0) / h)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor((np.asarray(x, np.float64) - x0) / h)


def plan(c, max_dst, budget=256 << 20):
    """(cells per pair slot, G): the host's plan of a call (icp.cpp grid_plan) - the tests aim points at cell borders with it."""
    n = 8
    while n < 2 * max(max_dst, 1):
        n <<= 1
    while n > 8 and max(c, 1) * n * 4 > budget:
        n >>= 1
    gc = 2
    while (gc + 1) ** 3 <= n:
        gc += 1
    return n, gc - 1
