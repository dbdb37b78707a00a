"""The singular-pair case builder (m2dp_svd_cases.py) checked on the CPU: the GPU test that uses it (test_gpu_m2dp_svd.py) can fail.

  families     : the counts of (variant, channel) matrices per band that the GPU test relies on, and the guards - every point 1e-6 bins from
                 every bin edge (the device's counts are the oracle's), a gap of 1.2 behind every tied group (its span is well defined);
  oracle       : for every matrix at s1/s2 >= 1.03 the oracle's one-sided Jacobi pair is LAPACK's pair within 1e-11, 100 x under the 1e-9 the
                 device is held to; measured 1.1e-14 at most.  Below 1.03 the two may differ (either may return any vector of the tied span),
                 which is why the GPU test compares named rows with the span and not with the oracle;
  restatement  : m2dp_svd_kernel's iteration and stop rule in numpy, as documentation of what the cases exercise.  It is not the oracle of any
                 device assertion.  On an exact tie the start vector G^256 * ones is the symmetric mix of the tied vectors, a fixed point of
                 u <- A A^T u: the iteration stops within 2 steps with u 0.16 to 0.23 (max-norm) from the oracle's vector - convergence alone cannot
                 name the row.  trace(G) after the normalised squarings tells: 1 for a unique pair, sqrt(j) for a j-fold tie."""
import numpy as np
import pytest

import gen_edge_cases as G
import m2dp_svd_cases as S
import oracle_lib

ORACLE_TOL = 1e-11


@pytest.fixture(scope="module")
def cases():
    return S.all_cases()


def _matrices(cases, bands):
    return [(c, v, ch) for c in cases for v in range(4) for ch in range(2) if c.band[v][ch] in bands]


def lapack_pair(A):
    """[u1 | v1] of numpy.linalg.svd with the project's sign rule sum(u) >= 0"""
    U, s, Vt = np.linalg.svd(A)
    sg = -1.0 if U[:, 0].sum() < 0 else 1.0
    return np.concatenate([sg * U[:, 0], sg * Vt[0]])


def kernel_restatement(A):
    """m2dp_svd_kernel in numpy (the sums in numpy's order, not the kernel's): u, v, polish steps taken, converged, trace(G^256)"""
    fro = (A * A).sum()
    if not fro > 0:
        u, v = np.zeros(64), np.zeros(128)
        u[0] = v[0] = 1.0
        return dict(u=u, v=v, steps=0, converged=True, trace=0.0)
    Gm = A @ A.T / fro
    for _ in range(8):
        Gm = Gm @ Gm
        Gm = Gm / np.sqrt((Gm * Gm).sum())
    u = Gm.sum(1)
    u = u / np.sqrt((u * u).sum())
    converged, sigma, steps = False, 0.0, 0
    for it in range(400):
        w = A @ (A.T @ u)
        nn = np.sqrt((w * w).sum())
        un = w / nn
        df = np.abs(un - u).max()
        u, sigma, steps = un, np.sqrt(nn), it + 1
        if df < 4e-15 and it >= 1:
            converged = True
            break
    v = A.T @ u / sigma
    sg = -1.0 if u.sum() < 0 else 1.0
    return dict(u=sg * u, v=sg * v, steps=steps, converged=converged, trace=float(np.trace(Gm)))


def test_families(cases):
    ties = _matrices(cases, ("tie",))
    assert len(ties) >= 4
    assert any(c.band[v] == ["tie", "tie"] for c in cases for v in range(4))               # count and intensity of one row both tie
    assert any(c.sv[v][ch][0] == c.sv[v][ch][2] for c, v, ch in ties)                          # a three-way tie
    near = sorted(c.ratio[v][ch] for c, v, ch in _matrices(cases, ("near",)))
    assert len(near) >= 4 and all(1 < r <= 1.01 for r in near)
    assert any(1 + 1e-9 < r < 1.0001 for r in near) and any(r > 1.005 for r in near)         # (1 + 1e-9: not a tie that LAPACK split by an ulp)
    assert sum(1.0001 <= r <= 1.005 for r in near) >= 2                                        # spread
    grey = [c.ratio[v][ch] for c, v, ch in _matrices(cases, ("grey",))]
    assert len(grey) >= 2 and all(1.01 < r < 1.03 for r in grey)
    slow = [c.ratio[v][ch] for c, v, ch in _matrices(cases, ("slow",))]
    assert len(slow) >= 6 and all(1.03 <= r < 1.05 for r in slow) and min(slow) < 1.035
    assert len(_matrices(cases, ("rank1",))) >= 1 and len(_matrices(cases, ("zero",))) >= 1
    for c, v, ch in _matrices(cases, ("zero",)):                                              # all intensities equal the average
        assert ch == 1 and (c.inten == c.frame[14]).all()
    # a batch needs rows of every class, and clouds no row of which can be named (the fillers of the batch-offset test)
    kinds = {c.row_class(v) for c in cases for v in range(4)}
    assert kinds == {"truth", "grey", "clean"} and len(S.clean_cases()) >= 3
    # no grey matrix beside a tied one in the same row: test_gpu_m2dp_svd.py's checks go by row, and such a channel would get the validity
    # check where it may deserve the oracle bound
    assert not any("grey" in c.band[v] and c.row_class(v) == "truth" for c in cases for v in range(4))
    assert len({c.name for c in cases}) == len(cases) and all(150 <= len(c.xyz) <= 250 for c in cases)


def test_guards(cases):
    for c in cases:
        assert G.m2dp_guard(c.aligned, c.max_rho).min() > G.GUARD_BINS, c.name
        assert np.array_equal(c.aligned, G.align(c.frame, c.xyz)) and np.array_equal(c.aligned, c.xyz)
        assert c.frame[13] == len(c.xyz) and c.frame[14] == float(oracle_lib.ave_intensity(c.inten))
    for c, v, ch in _matrices(cases, S.UNRESOLVED):
        s = c.sv[v][ch]
        k = S.tied_group(s)
        assert k >= 2 and S.gap_ok(s), (c.name, v, ch, s[:k + 1])
        assert s[k] <= s[0] / S.GAP_RATIO                                                      # (k < 64 here: there is a value behind the group)


def test_oracle_pair_is_lapacks_pair_where_it_is_unique(cases):
    worst = 0.0
    n = 0
    for c, v, ch in _matrices(cases, ("slow", "well", "rank1")):
        A = c.mats[v, ch]
        d = np.abs(c.rows[v, 192 * ch:192 * ch + 192] - lapack_pair(A)).max()                   # (rows: oracle_lib.top_singular_pair of mats)
        worst = max(worst, d)
        n += 1
        assert d < ORACLE_TOL, (c.name, v, ch, c.ratio[v][ch], d)
    print(f"oracle vs LAPACK over {n} matrices at s1/s2 >= 1.03: max |difference| = {worst:.2e} (bound {ORACLE_TOL:g})")
    for c, v, ch in _matrices(cases, ("zero",)):                                              # JacobiSVD of a zero matrix: identity factors
        want = np.zeros(192)
        want[0] = want[64] = 1.0
        assert np.array_equal(c.rows[v, 192 * ch:192 * ch + 192], want)


def test_restatement_of_the_kernels_rule_on_the_cases(cases):
    """what the cases exercise: an exact tie stops within 2 steps far from a singular vector (convergence alone does not name it) with
    trace(G) = sqrt(j); near ties run out of steps; the slow band needs more than 50 steps and still reaches LAPACK's pair"""
    for c, v, ch in _matrices(cases, ("tie",)):
        A = c.mats[v, ch]
        r = kernel_restatement(A)
        j = S.tied_group(c.sv[v][ch])
        assert r["converged"] and r["steps"] <= 2, (c.name, v, ch, r["steps"])
        assert abs(r["trace"] - np.sqrt(j)) < 1e-9, (c.name, v, ch, r["trace"], j)
        U = np.linalg.svd(A)[0][:, :j]
        assert np.linalg.norm(r["u"] - U @ (U.T @ r["u"])) < 1e-12                            # inside the tied span ...
        assert np.abs(r["u"] - c.rows[v, 192 * ch:192 * ch + 64]).max() > 0.1                   # ... and not the vector the oracle's sweeps end on
    for c, v, ch in _matrices(cases, ("near",)):
        r = kernel_restatement(c.mats[v, ch])
        # below 1.000007 a near tie converges like an exact one; from there to 1.01 400 steps are not enough
        assert (not r["converged"]) or c.ratio[v][ch] < 1.00001, (c.name, v, ch, c.ratio[v][ch], r["steps"])
        assert r["trace"] > 1.006, (c.name, v, ch, c.ratio[v][ch], r["trace"])                # (1 + t) / sqrt(1 + t^2), t = 1.01^-512
    steps = []
    for c, v, ch in _matrices(cases, ("slow",)):
        A = c.mats[v, ch]
        r = kernel_restatement(A)
        steps.append(r["steps"])
        assert r["converged"] and r["steps"] > 50, (c.name, v, ch, c.ratio[v][ch], r["steps"])
        assert r["trace"] - 1 < 1e-5, (c.name, v, ch, r["trace"])                             # 63 values at 1.03 would give 1.7e-5
        assert np.abs(np.concatenate([r["u"], r["v"]]) - lapack_pair(A)).max() < 1e-12
    print(f"slow band: {min(steps)} to {max(steps)} polish steps")
    for c, v, ch in _matrices(cases, ("well", "rank1")):
        r = kernel_restatement(c.mats[v, ch])
        assert r["converged"] and abs(r["trace"] - 1) < 1e-9
