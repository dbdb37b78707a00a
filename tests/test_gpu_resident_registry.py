"""The registry behind pr_gist_flagged_count / pr_delight_flagged_count (csrc/resident_match.cpp) is one table keyed by kind and
context: a context's last GIST match and its last DELIGHT match are remembered side by side, the last match of a kind wins, and a
database that is destroyed takes its entries with it.  Every matcher here runs with exact=True, so every query of a call is flagged
and the expected counts are the calls' query counts."""
import ctypes as C

import numpy as np
import pytest

from so_dso_place_recognition_amd import _lib, api, synth
from so_dso_place_recognition_amd.matcher import DelightMatcher, GistMatcher

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COLS = 32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def raw_count(ctx, kind, m):
    """pr_<kind>_flagged_count straight through the library: the count, or PRError"""
    c = C.c_int32(-1)
    ctx.check(getattr(ctx.lib, f"pr_{kind}_flagged_count")(ctx.h, int(m), C.byref(c)))
    return int(c.value)


def test_registry_is_per_kind_and_per_context_and_forgets_destroyed_databases():
    ctx = api.Context(0)
    gist_rows, delight_rows = synth.gist_signatures(7, 40, COLS), synth.delight_database(8, 20)
    gm = GistMatcher(8, 40, COLS, ctx=ctx, exact=True)
    dm = DelightMatcher(8, 20, ctx=ctx, exact=True)
    gm.pack_database(dev(gist_rows))
    dm.pack_database(dev(delight_rows))
    assert (gm.n, dm.n) == (40, 20)

    gm.match(dev(gist_rows[:3]))
    dm.match(dev(delight_rows[:2 * 16]))
    assert (gm.flagged_count(), dm.flagged_count()) == (3, 2)
    assert (dm.flagged_count(), gm.flagged_count()) == (2, 3)            # in either order of asking

    gm.match(dev(gist_rows[:5]))
    assert gm.flagged_count() == 5 and dm.flagged_count() == 2           # a GIST match leaves the DELIGHT entry alone

    dm.close()
    with pytest.raises(api.PRError) as err:
        raw_count(ctx, "delight", 2)
    assert err.value.code == _lib.PR_EINVAL and "pr_delight_flagged_count: m=2 is not the query count" in str(err.value)
    assert gm.flagged_count() == 5

    # two GIST databases on the context: the last match wins
    gm2 = GistMatcher(8, 40, COLS, ctx=ctx, exact=True)
    gm2.pack_database(dev(gist_rows[:11]))
    gm2.match(dev(gist_rows[:4]))
    assert gm2.flagged_count() == 4
    with pytest.raises(api.PRError) as err:
        gm.flagged_count()                                               # asks with its own m = 5
    assert err.value.code == _lib.PR_EINVAL
    gm.close()                                                           # not the database of the last match: the entry stays
    assert raw_count(ctx, "gist", 4) == 4
    gm2.close()                                                          # the database of the last match: the entry goes
    with pytest.raises(api.PRError) as err:
        raw_count(ctx, "gist", 4)
    assert err.value.code == _lib.PR_EINVAL and "(-1)" in str(err.value)
    ctx.close()
