"""The frame of the engine's per-request calls (set_call, infidex_amd/csrc/host/engine.cpp) on the GPU, across the seven features it carries: list_documents,
list_groups, range_facets, field_stats, field_quantiles, top_groups and field_distinct.

One corpus of 37 documents (two whole groups of sixteen and a partial one, four of them deleted) with an int64 column, a double column with a NaN, a string
column and two group columns.  Per feature ONE call of sixteen requests: refused ones at the first, a middle and the last position (an unknown field, a
filter with a syntax error, for the listings a limit of 0) between answered ones that repeat filters and interleave masks, value columns and group columns,
so that the device call orders them differently from the caller.  Every answered request equals the same request asked alone in a call of its own, every
refused one carries the message it gets alone, and the masks the call built plus the ones it reused are the distinct filters that compile.  Every comparison
is exact equality."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, ListRequest
from infidex_amd.engine import Session, GroupListRequest, RangeRequest, StatsRequest, QuantileRequest, TopGroupsRequest, DistinctRequest

pytestmark = pytest.mark.gpu

N = 37
A, B, C3 = "size >= 10", "shade = 'red'", "size < 30 AND shape != 'disc'"      # the filters that compile; None: every live document
BAD = "size = "                                                                # a syntax error
Q3 = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def engine():
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    size = (np.arange(N, dtype=np.int64) * 7) % 41 - 5
    price = ((np.arange(N) * 13) % 17).astype(np.float64) / 4 - 1.5; price[5] = np.nan
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(N)])
    e.set_column("size", size, facetable=False); e.set_column("price", price, facetable=False)
    e.set_column("name", ["n%02d" % ((i * 5) % 23) for i in range(N)], facetable=False)
    e.set_column("shade", (["red", "blue", "green"] * 13)[:N], facetable=True)
    e.set_column("shape", (["disc", "cube", "cone", "ring", "disc"] * 8)[:N], facetable=True)
    assert e.delete_documents([102, 116, 117, 136]) == 4
    return e


def held(ask, stats, reqs, refused, filters):
    """ask(reqs) in one call on a session of its own against ask([r]) per request on another; refused: place -> a word of its message."""
    together, alone = ask(reqs, 0), [ask([r], 1)[0] for r in reqs]
    built, reused = stats(0)[:2]
    assert len(reqs) == 16 and set(refused) >= {0, 15} and len(together) == 16
    for i, (t, a) in enumerate(zip(together, alone)):
        assert repr(t) == repr(a), (i, reqs[i], t, a)
        assert (t.error is not None) == (i in refused) and (i not in refused or refused[i] in t.error), (i, reqs[i], t)
    assert built + reused == filters and built == filters, (built, reused)
    again = ask(reqs, 0)
    assert [repr(t) for t in again] == [repr(t) for t in together] and stats(0)[:2] == (0, filters)


@pytest.fixture
def sessions(engine):
    both = [Session(engine), Session(engine)]      # fresh mask caches: one for the call of sixteen, one for the requests asked alone
    yield both
    for s in both:
        s.close()


def test_list_documents(engine, sessions):
    reqs = [ListRequest(A, "nosuch"), ListRequest(A, "size", True, 0, 5), ListRequest(B, "price", False, 2, 40), ListRequest(None, None, True, 30, 10),
            ListRequest(A, "price", True, 3, 4), ListRequest(C3, "name", False, 0, 40), ListRequest(B, "size", True, 0, 40), ListRequest(BAD, "size"),
            ListRequest(C3, "size", True, 1, 3), ListRequest(A, "size", False, 5, 5), ListRequest(None, "shade", False, 0, 40), ListRequest(B, "price", False, 0, 1),
            ListRequest(A, "size", True, 0, 0), ListRequest(C3, None, True, 2, 40), ListRequest(A, "name", True, 0, 40), ListRequest(B, "size", True, 0, 0)]
    held(lambda r, k: sessions[k].list_documents(r), lambda k: sessions[k].last_list_stats(), reqs, {0: "nosuch", 7: "syntax", 12: "limit", 15: "limit"}, 3)


def test_list_groups(engine, sessions):
    G = GroupListRequest
    reqs = [G(A, "shade", "size", True, 0, 0), G(A, "shade", "size", True, 0, 5), G(B, "shape", "price", False, 1, 40), G(None, "shape", None, True, 0, 10),
            G(A, "shape", "size", True, 0, 40), G(C3, "shade", "name", False, 0, 40), G(B, "shade", "size", True, 0, 40), G(A, "nosuch", "size"),
            G(C3, "shape", "size", False, 1, 3), G(A, "shade", "price", False, 0, 5), G(None, "name", "shade", False, 0, 40), G(B, "shape", "price", False, 0, 1),
            G(BAD, "shade", "size"), G(C3, "size", None, True, 2, 40), G(A, "shape", "name", True, 0, 40), G(B, "shade", "nosuch")]
    held(lambda r, k: sessions[k].list_groups(r), lambda k: sessions[k].last_group_list_stats(), reqs, {0: "limit", 7: "nosuch", 12: "syntax", 15: "nosuch"}, 3)


def test_range_facets(engine, sessions):
    R, ei, ed = RangeRequest, (-5, 0, 10, 36), (-1.5, 0.0, 1.25, 3.0)
    reqs = [R(A, "nosuch", ei), R(A, "size", ei), R(B, "price", ed), R(None, "size", (0, 1)), R(A, "price", ed), R(C3, "size", ei), R(B, "size", (-100, 100)),
            R(BAD, "size", ei), R(C3, "price", ed), R(A, "size", tuple(range(-5, 37))), R(None, "price", (-10.0, 10.0)), R(B, "price", ed), R(A, "name", ei),
            R(C3, "size", (3, 4)), R(A, "price", (0.0, 0.25)), R(B, "size", (5, 5))]
    held(lambda r, k: sessions[k].range_facets(r), lambda k: sessions[k].last_range_stats(), reqs, {0: "nosuch", 7: "syntax", 12: "string", 15: "increasing"}, 3)


def test_field_stats(engine, sessions):
    S = StatsRequest
    reqs = [S(A, "nosuch"), S(A, "size", "shade"), S(B, "price", "shape"), S(None, "size"), S(A, "price", "shade"), S(C3, "size", "shape"), S(B, "size"),
            S(BAD, "size", "shade"), S(C3, "price"), S(A, "size", "shape"), S(None, "price", "name"), S(B, "price", "shade"), S(A, "size", "nosuch"),
            S(C3, "size", "size"), S(A, "price"), S(B, "name")]
    held(lambda r, k: sessions[k].field_stats(r), lambda k: sessions[k].last_field_stats_stats(), reqs, {0: "nosuch", 7: "syntax", 12: "nosuch", 15: "string"}, 3)


def test_field_quantiles(engine, sessions):
    Q = QuantileRequest
    reqs = [Q(A, "nosuch"), Q(A, "size", Q3, "shade"), Q(B, "price", (0.5,), "shape"), Q(None, "size", Q3), Q(A, "price", Q3, "shade"), Q(C3, "size", (0.25, 0.75), "shape"),
            Q(B, "size", Q3), Q(BAD, "size", Q3, "shade"), Q(C3, "price", (0.9,)), Q(A, "size", (1.0, 0.0), "shape"), Q(None, "price", Q3, "name"), Q(B, "price", Q3, "shade"),
            Q(A, "size", ()), Q(C3, "size", Q3, "size"), Q(A, "price", (0.5, 0.5)), Q(B, "size", (1.5,))]
    held(lambda r, k: sessions[k].field_quantiles(r), lambda k: sessions[k].last_field_quantiles_stats(), reqs, {0: "nosuch", 7: "syntax", 12: "quantile", 15: "[0, 1]"}, 3)


def test_top_groups(engine, sessions):
    # (A, "size", "shade") is one table behind requests 1, 4, 8 and 11: several figures, both directions, three pages; 3 and 12 rank by size without a field
    T = TopGroupsRequest
    reqs = [T(A, "shade", "size", None, False, 0, 0), T(A, "shade", "sum", "size", False, 0, 5), T(B, "shape", "mean", "price", True, 0, 40), T(None, "shape", "size", None, False, 0, 10),
            T(A, "shade", "max", "size", True, 1, 1), T(C3, "name", "count", "price", False, 0, 40), T(A, "nosuch", "sum", "size"), T(B, "shade", "min", "size", False, 0, 40),
            T(A, "shade", "sum", "size", True, 0, 2), T(C3, "shape", "sum", "size", False, 2, 3), T(BAD, "shade", "sum", "size"), T(A, "shade", "mean", "size", False, 2, 5),
            T(None, "name", "size", None, True, 3, 7), T(B, "shape", "max", "price", False, 0, 1), T(A, "size", "min", "price", False, 0, 40), T(B, "shade", "sum", "nosuch")]
    held(lambda r, k: sessions[k].top_groups(r), lambda k: sessions[k].last_top_groups_stats(), reqs, {0: "limit", 6: "nosuch", 10: "syntax", 15: "nosuch"}, 3)


def test_field_distinct(engine, sessions):
    # 1 and 9 are one spec, apart; 10 and 13 are grouped by their own field; 2, 8 and 14 count the string column
    D = DistinctRequest
    reqs = [D(A, "nosuch"), D(A, "size", "shade"), D(B, "name", "shape"), D(None, "size"), D(A, "price", "shade"), D(C3, "size", "shape"), D(B, "size"),
            D(A, "size", "nosuch"), D(C3, "name"), D(A, "size", "shade"), D(None, "shade", "shade"), D(B, "price", "shade"), D(BAD, "size", "shade"),
            D(C3, "size", "size"), D(A, "name"), D(BAD, "name")]
    held(lambda r, k: sessions[k].field_distinct(r), lambda k: sessions[k].last_field_distinct_stats(), reqs, {0: "nosuch", 7: "nosuch", 12: "syntax", 15: "syntax"}, 3)
