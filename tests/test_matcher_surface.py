"""The Python surface of the three device-resident matchers (matcher.BowMatcher / GistMatcher / DelightMatcher): the public methods'
parameters - names, order, defaults, kinds - against a literal table, whichever class of the hierarchy defines them, and what each
class must inherit from where.  Importing the module needs no GPU."""
import inspect

import pytest

from so_dso_place_recognition_amd import matcher as M

SELECT = "self, mom_all, G, mask_width, p_weight, k, db_row0, q_row0"
MATCH = "self, queries, mask_width=0, k=1, db_row0=0, q_row0=0, group=None, force_exchange=False, mark=None"
CAPTURE = "self, queries, mask_width=0, k=1, db_row0=0, q_row0=0"
COMMON = {"pack_database": "self, rows", "reserve_database": "self, rows=None", "append_database": "self, rows", "local_phase1": "self, queries",
          "local_select": SELECT, "match": MATCH, "capture": CAPTURE}
TABLE = {
    "BowMatcher": dict(COMMON, __init__="self, max_queries, max_db, cols, n_words, ctx=None, device=None, max_postings=None",
                       on_new_stream="max_queries, max_db, cols, n_words, device=None, **kw"),
    "GistMatcher": dict(COMMON, __init__="self, max_queries, max_db, cols, ctx=None, device=None, exact=False",
                        on_new_stream="max_queries, max_db, cols, device=None, **kw"),
    "DelightMatcher": dict(COMMON, __init__="self, max_queries, max_db, ctx=None, device=None, exact=False",
                           on_new_stream="max_queries, max_db, device=None, **kw"),
    "Matcher": {"on_new_stream": "type_, max_queries, max_db, device=None"},
}
MARK = {inspect.Parameter.POSITIONAL_OR_KEYWORD: "", inspect.Parameter.VAR_KEYWORD: "**", inspect.Parameter.VAR_POSITIONAL: "*",
        inspect.Parameter.KEYWORD_ONLY: "kwonly:", inspect.Parameter.POSITIONAL_ONLY: "posonly:"}


def spelled(fn):
    """name, kind and default of every parameter, in order"""
    return ", ".join(MARK[p.kind] + p.name + ("" if p.default is inspect.Parameter.empty else f"={p.default!r}")
                     for p in inspect.signature(fn).parameters.values())


@pytest.mark.parametrize("cls,method", [(c, m) for c, t in TABLE.items() for m in t])
def test_public_method_takes_what_it_took(cls, method):
    assert spelled(getattr(getattr(M, cls), method)) == TABLE[cls][method]


def test_on_new_stream_is_a_classmethod_everywhere():
    for cls in TABLE:
        assert isinstance(inspect.getattr_static(getattr(M, cls), "on_new_stream"), classmethod)


def test_what_each_class_inherits():
    assert M.BowMatcher.flagged_count is M._Base.flagged_count                   # pr_order_flagged_count: BoW has no exact-row count
    for cls in (M.GistMatcher, M.DelightMatcher):
        assert isinstance(inspect.getattr_static(cls, "device_bytes"), property)
        assert cls.flagged_count is not M._Base.flagged_count and callable(cls.set_exact)
    assert not hasattr(M.BowMatcher, "device_bytes") and not hasattr(M.BowMatcher, "set_exact")
    for cls in (M.BowMatcher, M.GistMatcher, M.DelightMatcher):
        assert cls.plain is True and issubclass(cls, M._Base)
