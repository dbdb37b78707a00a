"""pr_moments_select_f64_dev (row moments and candidate selection in one sweep of the distances) against the two calls it replaces,
pr_row_moments_dev + pr_fuse_select_f64_dev: mom, idx, score and score64 must be equal BIT FOR BIT, whatever the rows hold and
whichever kernel the entry picks (the fused one for whole rows above the list size, the sliced / one-wave / short-row forms through the
two launchers).  The matrices are built on the host; no matcher launch is involved except in the last test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONTENTS = ("independent", "anti", "constant", "nan", "clusters", "overflow")
# (n, m) at which the entry runs the fused kernel's own list path (whole rows above the 4096-entry list that are neither sliced - fewer
# than 65 rows of 16384 columns or more - nor taken by the one-wave form - 64 rows or more of up to 32768 columns)
FUSED = {(4097, 3), (40000, 70), (40003, 70)}


def _rows(n, m, shift, seed):
    """Row r holds content CONTENTS[(r + shift) % 6]."""
    rng = np.random.default_rng(seed)
    dp = rng.random((m, n), dtype=np.float32)
    di = rng.random((m, n), dtype=np.float32)
    kinds = [CONTENTS[(r + shift) % len(CONTENTS)] for r in range(m)]
    for r, kind in enumerate(kinds):
        if kind == "anti":            # low d_p goes with high d_i: nothing is low in both, the corner cannot bound the k best
            di[r] = (1.0 - dp[r]) + rng.random(n, dtype=np.float32) * np.float32(1e-3)
        elif kind == "constant":      # sigma = 0 in one channel (rows r % 12 < 6) or in both
            dp[r] = np.float32(0.25)
            if r % 12 >= 6:
                di[r] = np.float32(0.5)
        elif kind == "nan":           # NaN columns (zero-norm signatures), a NaN first element included
            cols = rng.choice(n, size=max(1, n // 50), replace=False)
            dp[r, cols] = np.nan; di[r, cols] = np.nan
            dp[r, 0] = np.nan; di[r, 0] = np.nan
            if n > 7:
                di[r, 7] = np.nan     # NaN in one channel only
        elif kind == "clusters" and n >= 64:      # 5 copies of the best pair, then 40 copies of the next: the k-th place (9, 16) lies inside
            cols = rng.choice(n, size=min(45, n), replace=False)
            dp[r, cols[:5]] = np.float32(1e-3); di[r, cols[:5]] = np.float32(1e-3)
            dp[r, cols[5:]] = np.float32(2e-3); di[r, cols[5:]] = np.float32(2e-3)
        elif kind == "overflow" and n > 4096:     # the sampled head of the row is high, the rest low: the region takes in most of the row
            dp[r, 4096:] *= np.float32(0.01); di[r, 4096:] *= np.float32(0.01)
    return dp, di, kinds


def _bits(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def ctx():
    from so_dso_place_recognition_amd import api
    c = api.Context(0)
    yield c
    c.close()


NS, MS = (1, 3, 255, 4096, 4097, 20_011, 40_000, 40_003), (3, 70)
CASES = [(n, m, False) for n in NS for m in MS] + [(n, m, True) for n in NS for m in MS if (m * n) % 4]


@pytest.mark.parametrize("n,m,carved", CASES)
def test_one_call_equals_two_calls(ctx, n, m, carved):
    """carved: d_p and d_i cut from ONE allocation, starting one float past its base, where m n is not divisible by 4: the rows of
    the two matrices are then not co-aligned; otherwise two allocations, whose rows start at every alignment when n is odd (head != 0).
    k = 1, 9, 16 and mask 0 / 100 (with q_row0 = 37, db_row0 = 11) on every matrix."""
    import torch
    lib, h = ctx.lib, ctx.h
    P = lambda t: C.c_void_p(t.data_ptr())
    fell = C.c_int64(0)
    for shift in ((0, 3) if m < len(CONTENTS) else (0,)):
        dp, di, kinds = _rows(n, m, shift, 1000 * n + m + shift)
        if carved:
            buf = torch.zeros(2 * m * n + 8, dtype=torch.float32, device="cuda")
            a = buf[1:1 + m * n]; b = buf[1 + m * n:1 + 2 * m * n]
            a.copy_(torch.from_numpy(dp.ravel())); b.copy_(torch.from_numpy(di.ravel()))
        else:
            a = torch.from_numpy(dp).cuda(); b = torch.from_numpy(di).cuda()
        for k in (1, 9, 16):
            for mask, q0, d0 in ((0, 0, 0), (100, 37, 11)):
                out = []
                for one_call in (False, True):
                    mom = torch.full((m, 2, 3), -7.0, dtype=torch.float64, device="cuda")
                    idx = torch.full((m, k), -9, dtype=torch.int32, device="cuda")
                    sc = torch.full((m, k), -7.0, dtype=torch.float32, device="cuda")
                    s64 = torch.full((m, k), -7.0, dtype=torch.float64, device="cuda")
                    torch.cuda.synchronize()
                    if one_call:
                        ctx.check(lib.pr_select_fallback_rows(h, C.byref(fell)))
                        ctx.check(lib.pr_moments_select_f64_dev(h, P(a), P(b), m, n, P(mom), q0, d0, mask, 2.0, k, P(idx), P(sc), P(s64)))
                        ctx.check(lib.pr_select_fallback_rows(h, C.byref(fell)))
                    else:
                        ctx.check(lib.pr_row_moments_dev(h, P(a), P(b), m, n, P(mom)))
                        ctx.check(lib.pr_fuse_select_f64_dev(h, P(a), P(b), m, n, P(mom), 1, q0, d0, mask, 2.0, k, P(idx), P(sc), P(s64)))
                    ctx.sync()
                    out.append((mom, idx, sc, s64))
                what = f"n={n} m={m} carved={carved} shift={shift} k={k} mask={mask}"
                for name, x, y in zip(("mom", "idx", "score", "score64"), *out):
                    if _bits(x) != _bits(y):
                        bad = sorted({int(r) for r in np.nonzero((x.cpu().numpy().view(np.uint8).reshape(m, -1)
                                                                  != y.cpu().numpy().view(np.uint8).reshape(m, -1)).any(axis=1))[0]})
                        raise AssertionError(f"{name} differs ({what}) in rows {[(r, kinds[r]) for r in bad][:8]}")
                print(f"{what}: second-sweep rows {fell.value} of {m}")
                assert 0 <= fell.value <= m
                if (n, m) in FUSED and os.environ.get("PR_SELECT_FUSED") != "0":
                    # rows that cannot pass: the corner bounds nothing (anti), sigma = 0 (constant), the list overflows (n well above
                    # the sampled 4096 columns); rows that are not co-aligned: all of them
                    must = m if carved else sum(kd in ("anti", "constant") or (kd == "overflow" and n >= 20_000) for kd in kinds)
                    assert fell.value >= must, (what, fell.value, must)
                    assert shift != 0 or must > 0
                else:
                    assert fell.value == 0, what


_CHILD = r"""
import sys, numpy as np, torch
from so_dso_place_recognition_amd import api
from so_dso_place_recognition_amd.matcher import Matcher
n, m = 40000, 70
g = torch.Generator(device="cuda"); g.manual_seed(5)
db = torch.rand((n, 2400), dtype=torch.float64, device="cuda", generator=g)
db = db * (torch.rand((n, 2400), dtype=torch.float64, device="cuda", generator=g) < 0.3)
q = db[torch.arange(m, device="cuda") * 531 + 17].clone()
q = q * (torch.rand((m, 2400), dtype=torch.float64, device="cuda", generator=g) < 0.9)
mt = Matcher("sc", m, n, ctx=api.Context(0))
mt.pack_database(db)
res = {}
for k, mask in ((1, 0), (5, 100)):
    idx, sc = mt.match(q, mask, 2.0, k)
    torch.cuda.synchronize()
    res[f"idx{k}"] = idx.cpu().numpy(); res[f"sc{k}"] = sc.cpu().numpy(); res[f"mom{k}"] = mt._bufs["mom"].cpu().numpy()
np.savez(sys.argv[1], **res)
"""


def test_matcher_same_with_switch_either_way(tmp_path):
    """Matcher.match at n = 40 000, m = 70 (whole rows, the fused kernel) with PR_SELECT_FUSED=1 and =0 - the switch is read once per
    process, hence two of them: indices, scores and the moments the re-evaluation used, byte for byte."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for v in ("1", "0"):
        path = str(tmp_path / f"fused{v}.npz")
        env = dict(os.environ, PR_SELECT_FUSED=v, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        subprocess.run([sys.executable, "-c", _CHILD, path], check=True, env=env, cwd=root, timeout=300)
        outs.append(np.load(path))
    assert set(outs[0].files) == set(outs[1].files) and len(outs[0].files) == 6
    for name in outs[0].files:
        assert outs[0][name].tobytes() == outs[1][name].tobytes(), name
    assert (outs[0]["idx1"][:, 0] == np.arange(70) * 531 + 17).all()
