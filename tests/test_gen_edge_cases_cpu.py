"""The edge-case builder (gen_edge_cases.py) checked on the CPU: the GPU test that uses it (test_gpu_gen_edges.py) can fail.

  mutation     : every near-edge probe, mirrored alone to the other side of its edge, changes the oracle's signature (SC / DELIGHT: an
                 element differs; M2DP: by >= 1000 x the GPU tolerance of 1e-9 in max-norm) - a kernel that bins one probe on the wrong side
                 cannot pass;
  guards       : in longdouble, no base point within 1e-6 bins of an SC / M2DP edge or 1e-6 m of a DELIGHT octant plane / the 10 m sphere,
                 no near-edge probe closer than 1e-11 bins to its edge (the device atan2 may differ from glibc's in the last ulp: < 1e-13 bins);
  conditioning : the two leading singular values of all eight matrices of every M2DP case are a factor >= 1.05 apart.  m2dp_svd_kernel names
                 a row on a (nearly) exact tie (trace of the squared Gram matrix, s1/s2 < 1.0136) and when 8 squarings of the Gram
                 matrix and 400 polish steps have not brought the change of u below 4e-15, i.e. when (s2/s1)^(2*256 + 2*400) > 4e-15,
                 s1/s2 < 1.026; 1.05 is inside the converging side.
                 (Everything below 1.05 - ties, near ties, the slow band - is m2dp_svd_cases.py / test_gpu_m2dp_svd.py's subject.)"""
import numpy as np
import pytest

import gen_edge_cases as G
import oracle_lib

GPU_TOL_M2DP = 1e-9


@pytest.fixture(scope="module")
def cases():
    return G.all_cases()


def _sig(case, al):
    if case.kind == "sc":
        return oracle_lib.sc_signature_aligned(al, case.inten, case.max_rho)
    return oracle_lib.delight_signature_aligned(al, case.inten).reshape(-1)


@pytest.mark.parametrize("kind", ["sc", "delight"])
def test_mirroring_one_probe_changes_the_oracle_signature(cases, kind):
    n = 0
    for c in cases[kind]:
        ref = _sig(c, c.aligned)
        for pr in c.probes:
            _, al = G.mutated(c, pr)
            mut = _sig(c, al)
            assert not np.array_equal(ref, mut), (c.name, pr["edge"], pr["offset"])
            if kind == "sc":        # the builder's promise: structure AND binarised intensity of both bins change
                d = np.nonzero(ref != mut)[0]
                assert (d < 1200).sum() >= 2 and (d >= 1200).sum() >= 2, (c.name, pr["edge"], pr["offset"], d)
            n += 1
    assert n >= (1600 if kind == "sc" else 80)


def test_mirroring_one_m2dp_probe_moves_the_signature_by_1000_tolerances(cases):
    n = 0
    for c in cases["m2dp"]:
        cm, _ = oracle_lib.m2dp_matrices(c.aligned, c.inten, c.max_rho, 1, 1)       # the variant the probes are placed in
        ref = oracle_lib.top_singular_pair(cm)
        for pr in c.probes:
            _, al = G.mutated(c, pr)
            cm2, _ = oracle_lib.m2dp_matrices(al, c.inten, c.max_rho, 1, 1)
            assert np.abs(cm2 - cm).sum() >= 1, (c.name, pr["edge"])                 # the probe left its bin (ring edge 8: for the dropped side)
            d = np.abs(oracle_lib.top_singular_pair(cm2) - ref).max()                # 192 of the signature's elements
            assert d >= 1000 * GPU_TOL_M2DP, (c.name, pr["edge"], pr["offset"], d)
            n += 1
    assert n >= 280


def test_guard_distances(cases):
    for c in cases["sc"]:
        d = G.sc_guard(c.aligned, c.max_rho)
        quiet = (c.role == "base") | (c.role == "anchor") | (c.role == "lone")
        assert quiet.sum() == 0 or d[quiet].min() > G.GUARD_BINS, c.name
        assert c.role[c.role == "anchor"].size == 0 or d[c.role == "anchor"].min() >= 0.2, c.name
        ts, tr = G.sc_bin_coords(c.aligned, c.max_rho)
        for pr in c.probes:
            own = G.edge_dist(ts if pr["edge"][0] == "sector" else tr)[pr["index"]]
            assert G.MIN_PROBE_BINS <= own <= abs(pr["offset"]) * 1.1 + 1e-13, (c.name, pr["edge"], pr["offset"], own)
            assert d[pr["index"]] >= G.MIN_PROBE_BINS
            _, al = G.mutated(c, pr)
            assert G.sc_guard(al[pr["index"]][None], c.max_rho)[0] >= G.MIN_PROBE_BINS
    for c in cases["m2dp"]:
        d = G.m2dp_guard(c.aligned, c.max_rho)
        quiet = (c.role == "base") | (c.role == "lone")
        assert quiet.sum() == 0 or d[quiet].min() > G.GUARD_BINS, c.name
        for pr in c.probes:
            edge, k, plane = pr["edge"]
            ts, tr = G.m2dp_bin_coords(c.aligned[pr["index"]][None], 3, c.max_rho)
            own = G.edge_dist(ts if edge == "sector" else tr)[plane, 0]
            assert G.MIN_PROBE_BINS <= own <= abs(pr["offset"]) * 1.1 + 1e-13, (c.name, pr["edge"], pr["offset"], own)
            assert d[pr["index"]] >= G.MIN_PROBE_BINS, (c.name, pr["edge"])         # ... nor that close to any other plane's edge
    for c in cases["delight"]:
        d = G.delight_guard(c.aligned)
        assert (c.role == "base").sum() == 0 or d[c.role == "base"].min() > G.GUARD_M, c.name
        # 1e-12 away from the float rounding midpoints next to 10 (the spacing of float at 10 is 2^-20)
        r = np.sqrt((c.aligned.astype(np.longdouble) ** 2).sum(1))
        for mid in (10 + 2.0 ** -21, 10 - 2.0 ** -21):
            assert np.abs(r - np.longdouble(mid)).min() > 1e-12


def test_m2dp_cases_are_well_conditioned(cases):
    for c in cases["m2dp"]:
        _, mats = oracle_lib.m2dp_signature_aligned(c.aligned, c.inten, c.max_rho, with_matrices=True)
        for v in range(4):
            for ch in range(2):
                s = np.linalg.svd(mats[v, ch], compute_uv=False)
                assert s[0] == 0 or s[0] >= 1.05 * s[1], (c.name, v, ch, s[:2])


def test_cases_hold_what_they_are_built_for(cases):
    sizes = {k: sorted({len(c.xyz) for c in cases[k]}) for k in cases}
    assert sizes["sc"] == [1, 511, 513, 1537, 2049] and sizes["delight"] == [1, 511, 513, 1537, 2049]
    assert sizes["m2dp"] == [1, 255, 257, 1024, 1025, 2000]
    for k in cases:
        for c in cases[k]:
            assert np.array_equal(c.aligned, G.align(c.frame, c.xyz)) and c.frame[13] == len(c.xyz) and c.frame[15] == 1.0
            assert c.frame[14] == float(oracle_lib.ave_intensity(c.inten))
            if c.frame_kind == "identity":
                assert np.array_equal(c.aligned, c.xyz)                              # (-0 == +0 here; the signs are what align() makes of them)
            else:
                R = c.frame[3:12].reshape(3, 3)
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and np.abs(R).min() > 0.05          # not axis-aligned
            if len(c.probes) > 4:                                                     # near probes sit at the first and the last index
                idx = {p["index"] for p in c.probes}
                assert 0 in idx and len(c.xyz) - 1 in idx
    for c in cases["sc"]:
        s = oracle_lib.sc_signature_aligned(c.aligned, c.inten, c.max_rho)
        if c.name.startswith("sc_one"):
            assert not s.any()                                                        # one point: max - min = 0 and mean == average
        if c.name.startswith("sc_exact"):
            ts, tr = G.sc_bin_coords(c.aligned)
            lone = np.nonzero((np.floor(ts) == 44) & (np.floor(tr) == 17))[0]
            assert len(lone) == 1 and c.role[lone[0]] == "lone" and c.inten[lone[0]] == c.frame[14]
            assert s[c.lone_bin] == 0.0 and s[1200 + c.lone_bin] == 0.0             # alone in its bin, mean == average: the strict > gives 0
        if c.name == "sc_exact_ide":                                                  # si == 60 (atan2 = +pi exactly) and si == 0 from -0 both occur
            y, z = c.aligned[:, 1], c.aligned[:, 2]
            si = np.floor((np.arctan2(z, y) + np.pi) * (60 / (2.0 * np.pi))).astype(int)
            assert (si == 60).any() and ((si == 0) & (z == 0) & np.signbit(z) & (y < 0)).any()
    for c in cases["m2dp"]:
        if len(c.xyz) > 1 and c.frame_kind == "identity":                             # si == 16 (atan2 = +pi exactly) occurs in every variant
            for v in range(4):
                xp, yp = G.m2dp_proj(c.aligned, v)
                assert (np.floor((np.arctan2(yp, xp) + np.pi) * (16 / (2.0 * np.pi))) == 16).any(), (c.name, v)
        if len(c.xyz) == 257:
            assert (c.inten < 0).any()                                                # the EXACT accumulation
        elif len(c.xyz) > 1:
            assert (c.inten >= 0).all()
        if len(c.xyz) > 1:                                                            # bins whose mean equals the float average exactly
            lone = int(np.nonzero(c.role == "lone")[0][0])
            ave = c.frame[14]
            assert c.inten[lone] == ave and ave != np.rint(ave)
            tie_groups, lone_zero = set(), 0
            for v, (dx, dy) in enumerate(oracle_lib.M2DP_VARIANTS):
                cm, im = oracle_lib.m2dp_matrices(c.aligned, c.inten, c.max_rho, dx, dy)
                idx = G._m2dp_idx(c.aligned, v, c.max_rho)
                for k in range(64):
                    ok = (idx[k] >= 0) & (idx[k] < 128)
                    sm = np.bincount(idx[k][ok], weights=c.inten[ok].astype(np.float64), minlength=128)
                    assert np.array_equal(np.bincount(idx[k][ok], minlength=128), cm[k])
                    tie = (cm[k] > 0) & (sm == cm[k] * ave)
                    if tie.any():
                        tie_groups.add((v, k // 16))
                        assert tie.sum() == 1 and idx[k][lone] == np.nonzero(tie)[0][0] and cm[k][tie][0] == 1    # the lone point's bin, alone
                        assert im[k][tie][0] == 0.0                                                            # strict >: 0
                        lone_zero += 1
            assert lone_zero >= 1 and len(tie_groups) == c.lone_groups
            if len(c.xyz) >= 1024:
                # m2dp_bin_kernel reruns a workgroup ((variant, 16 planes) in the 16-plane form) with the exact accumulation when a bin ties
                # with the average; these clouds have no negative intensity, so every other workgroup stays in the FAST mode
                assert len(tie_groups) <= 4, (c.name, tie_groups)
    for c in cases["delight"]:
        if len(c.xyz) > 1:
            f = c.aligned.astype(np.float32)
            assert (c.aligned == 5e-324).any() and ((f == 0) & (c.aligned > 0)).any() and (f == np.float32(1e-45)).any()
            assert set(np.float32(G.DELIGHT_INTEN)) <= set(c.inten)
