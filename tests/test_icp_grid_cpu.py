"""CPU-side checks of the uniform-grid correspondence search (csrc/icp_grid.hip, icp.cpp): the header declares the four
new entry points and _lib.py binds them with matching signatures and constants; argument errors are PR_EINVAL before any device is
touched; the premise - a refinement on correspondences masked to d2 < max_corr^2 is the unmasked refinement bit for bit - holds for
every committed case in the restatement; and the containment margin: with the cell edge and the cell coordinate as the source states
them, d2 < max_corr^2 implies a cell-index difference of at most 1, for coordinates up to the stated bound and distances within a few
ulps of max_corr."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_cases
import icp_grid_np
import icp_np
from so_dso_place_recognition_amd import _lib
from test_icp_cpu import _ctype, _declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "so_dso_place_recognition_amd", "csrc")
NEW = ("pr_set_icp_search", "pr_get_icp_search", "pr_icp_nn_radius_dev", "pr_icp_nn_radius")


def test_header_declares_the_four_symbols_and_lib_binds_them():
    decls = _declarations()
    lib = _lib.load()
    for name in NEW:
        assert name in decls, name
        assert hasattr(lib, name), name                                  # exported by the shared library
        res, args = _lib.SYMBOLS[name]
        want = [_ctype(a) for a in decls[name][1].split(",")]
        got = [C.c_void_p if (a is C.c_void_p or hasattr(a, "contents")) else a for a in args]
        assert got == want, (name, got, want)
        assert res is _ctype(decls[name][0] + " x")
    for name, ref in (("pr_icp_nn_radius_dev", "pr_icp_nn_dev"), ("pr_icp_nn_radius", "pr_icp_nn")):      # the brute-force pass's arguments + max_corr
        names = re.findall(r"(\w+)\s*[,)]", decls[name][1] + ")")
        base = re.findall(r"(\w+)\s*[,)]", decls[ref][1] + ")")
        assert [n for n in names if n != "max_corr"] == base and names.count("max_corr") == 1 and names.index("max_corr") == len(names) - 4


def test_constants_equal_the_headers():
    hdr = open(os.path.join(ROOT, "include", "place_recognition.h")).read()
    for word, value in (("BRUTE", 0), ("GRID", 1)):
        assert re.search(rf"#define PR_ICP_SEARCH_{word} {value}\b", hdr) and getattr(_lib, "ICP_SEARCH_" + word) == value


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_argument_errors_are_einval_without_a_device():
    lib = _lib.load()
    assert lib.pr_set_icp_search(None, 0) == _lib.PR_EINVAL
    assert lib.pr_set_icp_search(None, 1) == _lib.PR_EINVAL
    assert lib.pr_get_icp_search(None) == _lib.PR_EINVAL
    x = np.zeros((8, 3)); o = np.array([0, 4, 8], np.int64); ps = np.zeros(2, np.int32); T = np.zeros((2, 3, 4))
    oo = np.zeros(3, np.int64); ji = np.zeros(8, np.int32); dd = np.zeros(8)

    def err(rc, word):
        assert rc == _lib.PR_EINVAL
        assert word in lib.pr_last_error(None).decode(), (word, lib.pr_last_error(None))

    def opt(a):
        return _p(a) if a is not None else None

    def dev(xq=x, oq=o, Nq=2, c=2, T_=T, ms=4, md=4, mc=1.0, out=oo, nj=ji):
        return lib.pr_icp_nn_radius_dev(None, opt(xq), opt(oq), Nq, _p(x), _p(o), 2, _p(ps), _p(ps), c, opt(T_), ms, md, mc, opt(out), opt(nj), _p(dd))

    def host(Nq=2, c=2, T_=T, oq=o, mc=1.0, out=oo):
        return lib.pr_icp_nn_radius(None, _p(x), opt(oq), Nq, _p(x), _p(o), 2, _p(ps), _p(ps), c, opt(T_), mc, opt(out), _p(ji), _p(dd))

    for kw in (dict(Nq=-1), dict(c=-1), dict(ms=-1), dict(md=-3)):
        err(dev(**kw), "negative")
    for kw in (dict(xq=None), dict(oq=None), dict(T_=None), dict(out=None), dict(nj=None)):
        err(dev(**kw), "NULL")
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        err(dev(mc=bad), "max_corr")
        err(host(mc=bad), "max_corr")
    err(dev(), "ctx")
    err(host(Nq=-1), "negative"); err(host(c=-2), "negative"); err(host(T_=None), "NULL"); err(host(oq=None), "NULL"); err(host(out=None), "NULL")
    err(host(), "ctx")


@pytest.mark.parametrize("name", list(icp_cases.CASES))
def test_premise_masked_correspondences_give_the_same_refinement_bit_for_bit(name):
    c, ref = icp_cases.case(name), icp_cases.reference(name)
    got = icp_grid_np.icp_masked(c["P"], c["Q"], c["T0"], **icp_cases.PARAMS)
    assert got["T"].tobytes() == ref["T"].tobytes()
    for key in ("status", "iters", "n_inl"):
        assert got[key] == ref[key], key
    assert np.float64(got["fitness"]).tobytes() == np.float64(ref["fitness"]).tobytes()
    assert np.float64(got["rmse"]).tobytes() == np.float64(ref["rmse"]).tobytes()
    Pt = icp_np.transform(c["T0"], c["P"])                               # and the mask does mask something in these cases
    idx, d2 = icp_grid_np.nn_radius(Pt, c["Q"], icp_cases.MAX_CORR)
    assert (idx < 0).any() and (idx >= 0).any() and np.all(np.isinf(d2[idx < 0])) and np.all(d2[idx >= 0] < icp_cases.MAX_CORR ** 2)


def test_grid_formulas_restate_the_source_text():
    hip = open(os.path.join(CSRC, "icp_grid.hip")).read()
    hpp = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert re.search(r"constexpr double ICP_GRID_SLACK = 1\.0 \+ 0x1p-10;", hpp) and icp_grid_np.SLACK == 1.0 + 2.0 ** -10
    edge = re.search(r"double cell_edge\(double max_corr, double ext, int G\) \{ return (.*?); \}", hip).group(1)
    coord = re.search(r"double cell_coord\(double x, double x0, double h\) \{ return (.*?); \}", hip).group(1)
    assert edge == icp_grid_np.cell_edge.__doc__ and coord == icp_grid_np.cell_coord.__doc__
    assert len(re.findall(r"cell_edge\(", hip)) == 2                     # one definition, one use: the box kernel
    assert "cell_coord(p[a], B.x0[a], B.h)" in hip and hip.count("floor(") == 1      # source and target cells come from the one formula


def test_containment_margin_at_the_radius():
    """10^5 (target, source) coordinate pairs per trial set: x0, the extent and max_corr of magnitudes up to the stated bound, the
    source a few ulps either side of max_corr away from the target.  Whenever d2 < max_corr^2 - on the rounded values, as the kernels
    form it - the two cell coordinates differ by at most 1, so the source's 27 cells hold the target."""
    rng = np.random.default_rng(7)
    n = 100000
    seen_in = seen_out = 0
    for trial in range(4):
        with np.errstate(over="ignore", invalid="ignore"):
            e_hi = np.log2(icp_grid_np.COORD_BOUND)
            mc = np.ldexp(1.0 + rng.random(n), rng.integers(-40, int(e_hi), n))
            G = rng.integers(1, 1 << 12, n).astype(np.float64)
            if trial == 0:            # max_corr sets h: a small cloud next to its box
                ext = mc * rng.random(n) * G
                x0 = rng.normal(0, 1, n) * mc * 4
            elif trial == 1:          # the extent sets h
                ext = mc * G * (1 + 100 * rng.random(n))
                x0 = rng.normal(0, 1, n) * ext
            elif trial == 2:          # a box far from the origin: coordinates much larger than the extent
                ext = mc * G * rng.random(n) * 2
                x0 = np.ldexp(1.0 + rng.random(n), rng.integers(0, int(e_hi), n)) * rng.choice([-1.0, 1.0], n)
            else:                     # unit-scale clouds, max_corr = 1 and lattice-like coordinates
                mc = np.ones(n); ext = rng.integers(0, 200, n).astype(np.float64); x0 = rng.integers(-100, 100, n).astype(np.float64)
            ok = (np.abs(x0) <= icp_grid_np.COORD_BOUND) & (np.abs(x0 + ext) <= icp_grid_np.COORD_BOUND) & np.isfinite(ext)
            q = x0 + ext * rng.random(n)
            q = np.where(trial == 3, np.round(q), q)
            q = np.clip(q, x0, x0 + ext)
            ext = np.maximum(ext, q - x0)
            h = icp_grid_np.cell_edge(mc, ext, G)
            p = q + mc * rng.choice([-1.0, 1.0], n)
            for _ in range(int(rng.integers(0, 4))):
                p = np.nextafter(p, np.where(rng.random(n) < 0.5, q, np.where(p > q, np.inf, -np.inf)))
            dx = p - q
            d2 = ((dx * dx) + 0.0 * 0.0) + 0.0 * 0.0
            inl = ok & np.isfinite(p) & (d2 < mc * mc)
            tq, tp = icp_grid_np.cell_coord(q, x0, h), icp_grid_np.cell_coord(p, x0, h)
        assert np.all((tq[ok] >= 0) & (tq[ok] <= G[ok]))                 # a target's cell: at most G + 1 per axis
        assert np.all(np.abs(tp[inl] - tq[inl]) <= 1), np.flatnonzero(inl & ~(np.abs(tp - tq) <= 1))[:5]
        assert np.all((tp[inl] >= -1) & (tp[inl] <= G[inl] + 1))         # and the probe's range test keeps every inlier's source
        seen_in += int(inl.sum()); seen_out += int((ok & ~inl).sum())
    assert seen_in > 50000 and seen_out > 50000
