"""SearchEngine.range_facets on the GPU: bucket counts, below / above / NaN counts, total and min / max of a numeric field over a filter.

The expected answer is plain numpy on the column's VALUES and uses no ranks: which documents a filter accepts comes from the oracle's filter VM
(FilteredModel.accept of tests/test_gpu_filtered_facets.py) and the Deleted flags; j = np.searchsorted(edges, v, side="right") over the members that are
not NaN gives below (j = 0), the buckets (1 .. B) and above (B + 1); int columns stay in int64 throughout.  Every comparison is exact equality, min and
max included.

The corpus, columns and filters are those of tests/test_gpu_list_documents.py (70 001 documents: 4375 groups of 16 and a partial one of a single
document): shop (int, 100 values, 99 only at the last document), year (int), rating (double with NaN, -0.0 and 0.0), wide (55 000 values), uniq
(every value distinct, multiples of three less 5000: there are integers strictly between its values)."""
import numpy as np
import pytest

from infidex_amd import RangeFacets, RangeRequest
from infidex_amd.engine import Session
from tests.test_gpu_list_documents import D, FILTERS, ONE_PCT, NOTHING, EVERYTHING, LAST_ONLY, TWO_COLS, fx, variant, variantless      # noqa: F401 (fx: the module's fixture)

pytestmark = pytest.mark.gpu

FIELDS = ["shop", "year", "rating", "wide", "uniq"]


def members(m, x):
    """bool per document: live and accepted"""
    return ~m.fm.deleted if x is None else (m.fm.accept(variantless(x)) & ~m.fm.deleted)


def expect(m, r):
    """the contract on the values, no ranks"""
    live = members(m, r.filter)
    v = np.asarray(m.cols[r.field][0])[live]
    nan = 0
    if v.dtype.kind == "f":
        edges = np.asarray(r.edges, np.float64)
        nan = int(np.isnan(v).sum()); v = v[~np.isnan(v)]
    else:
        assert v.dtype == np.int64
        edges = np.asarray(r.edges, np.int64)
    j = np.searchsorted(edges, v, side="right")
    c = np.bincount(j, minlength=len(edges) + 1)
    lo = hi = None
    if len(v):
        lo, hi = (float(v.min()), float(v.max())) if v.dtype.kind == "f" else (int(v.min()), int(v.max()))
    return RangeFacets(tuple(r.edges), [int(x) for x in c[1:-1]], int(c[0]), int(c[-1]), nan, int(live.sum()), lo, hi, None)


def check(m, got, r, ctx=None):
    want = expect(m, r)
    assert got.error is None, (ctx, r, got.error)
    assert got.nan + got.below + sum(got.counts) + got.above == got.total, (ctx, r, got)
    assert len(got.counts) == len(r.edges) - 1
    assert (got.total, got.nan, got.below, got.above) == (want.total, want.nan, want.below, want.above), (ctx, r.filter, r.field, r.edges[:4], got.total, got.nan, got.below, got.above, want.total, want.nan, want.below, want.above)
    assert got.counts == want.counts, (ctx, r.filter, r.field, r.edges[:4], got.counts[:8], want.counts[:8])
    assert got.min == want.min and got.max == want.max and type(got.min) is type(want.min) and type(got.max) is type(want.max), (ctx, r.filter, r.field, got.min, got.max, want.min, want.max)
    assert tuple(got.edges) == tuple(r.edges)


def run(s, m, reqs, ctx=None):
    got = s.range_facets(reqs)
    assert len(got) == len(reqs)
    for g, r in zip(got, reqs):
        check(m, g, r, ctx)
    return got


def edge_sets(vals):
    """name -> edges for a column of these values, from the whole column (whatever a filter leaves of it)"""
    vals = np.asarray(vals)
    isf = vals.dtype.kind == "f"
    u = np.unique(vals[~np.isnan(vals)]) if isf else np.unique(vals)
    n = len(u)
    assert n >= 8
    cast = float if isf else int
    lo, hi = cast(u[0]), cast(u[-1])
    out = {"one bucket": (cast(u[n // 4]), cast(u[3 * n // 4]))}
    if isf:
        out["256 buckets"] = tuple(float(x) for x in np.linspace(lo - 0.5, hi + 0.5, 257))
    else:
        step = max(1, (hi - lo + 20) // 256 + 1)
        out["256 buckets"] = tuple(lo - 10 + i * step for i in range(257))
        assert out["256 buckets"][-1] > hi
    out["at values"] = tuple(cast(u[i]) for i in (0, n // 3, 2 * n // 3, n - 1))     # v == e_i opens bucket i; v == e_B is above
    gaps = np.nonzero(np.diff(u) >= (0 if isf else 3))[0]                           # neighbours with room for two edges strictly between them
    if isf:
        k = n // 2
        out["between values"] = tuple(float((u[i] + u[i + 1]) / 2) for i in (0, n // 3, k, n - 2))
        out["adjacent, nothing between"] = (lo, float(np.nextafter(u[k], np.inf)), float(u[k + 1]), hi)
        assert all(a < b for a, b in zip(out["between values"], out["between values"][1:])) and not np.isin(out["between values"], u).any()
    elif len(gaps):
        g = [int(gaps[0]), int(gaps[len(gaps) // 2]), int(gaps[-1])]
        out["between values"] = tuple(sorted(set(int(u[i]) + 1 for i in g)))
        k = g[1]
        out["adjacent, nothing between"] = tuple(sorted({lo, int(u[k]) + 1, int(u[k]) + 2, hi}))
        if len(out["between values"]) < 2:
            out["between values"] += (hi + 5,)
    else:                                                                            # consecutive integers: no integer lies strictly between two values
        out["adjacent, nothing between"] = (cast(u[n // 2]), hi + 1, hi + 2)
    out["all below"] = (lo - 30, lo - 20, lo - 10)
    out["all above"] = (hi + 10, hi + 20, hi + 30)
    return out


def test_every_filter_field_and_edge_set(fx):
    e, m, _ = fx
    assert 500 <= int(members(m, ONE_PCT).sum()) <= 900 and np.nonzero(members(m, LAST_ONLY))[0].tolist() == [D - 1] and D % 16 == 1
    s = Session(e)
    try:
        sets = {f: edge_sets(m.cols[f][0]) for f in FIELDS}
        assert "between values" in sets["uniq"] and "between values" in sets["rating"]
        sets["rating"]["both zeros"] = (float("-inf"), 0.0, float("inf"))
        bys = {}
        for f in FIELDS:
            reqs = [RangeRequest(x, f, ed) for x in FILTERS for ed in sets[f].values()]
            got = run(s, m, reqs, f)
            assert s.last_range_stats()[2] == 1
            by = bys[f] = {(r.filter, name): g for (r, g), name in zip(zip(reqs, got), [n for _ in FILTERS for n in sets[f]])}
            for x in FILTERS:
                assert by[(x, "all below")].below == 0 and sum(by[(x, "all below")].counts) == 0 and by[(x, "all above")].above == 0
                assert by[(x, "adjacent, nothing between")].counts[1] == 0         # the bucket between the two adjacent edges
                t = by[(x, "256 buckets")]
                assert len(t.counts) == 256 and t.below == 0 and t.above == 0
            # the half-open sides: the smallest value opens bucket 0, the largest is at e_B and so above
            a = by[(None, "at values")]
            assert a.below == 0 and a.above >= 1 and a.counts[0] >= 1 and a.min == a.edges[0] and a.max == a.edges[-1]
        # the double column's specials: both zeros in [0, inf), NaN in `nan` only
        rating = np.asarray(m.cols["rating"][0])
        z = bys["rating"][(None, "both zeros")]
        assert z.nan == int(np.isnan(rating).sum()) > 0 and z.below == 0 and z.above == 0
        assert z.counts == [int((rating < 0).sum()), int((rating >= 0).sum())] and int((rating == 0).sum()) >= 2 and np.signbit(rating[rating == 0]).any()
        assert z.counts[1] - s.range_facets(None, "rating", (float("-inf"), float(np.nextafter(0.0, 1.0)), float("inf"))).counts[1] == int((rating == 0).sum())
        # particular filters: the partial last group alone; nothing at all
        last = s.range_facets(LAST_ONLY, "shop", (0, 50, 99, 100))
        assert (last.total, last.counts, last.below, last.above, last.min, last.max) == (1, [0, 0, 1], 0, 0, 99, 99)
        for f in FIELDS:
            none = s.range_facets(NOTHING, f, sets[f]["one bucket"])
            assert (none.total, none.counts, none.below, none.above, none.nan, none.min, none.max, none.error) == (0, [0], 0, 0, 0, None, None, None)
        # total is the size of the set the rest of the family counts
        for x in FILTERS:
            t = s.range_facets(x, "year", (1950, 2000)).total
            assert t == s.list_documents(x).total == int(members(m, x).sum())
            if x is not None:
                assert t == s.facets_of_documents(x).total
    finally:
        s.close()


def sixteen(m):
    four = [variant(x, 3) for x in (ONE_PCT, EVERYTHING, TWO_COLS, LAST_ONLY)]
    sets = {f: list(edge_sets(m.cols[f][0]).values()) for f in FIELDS}
    return [RangeRequest(four[(i * 3) % 4], FIELDS[i % 5], sets[FIELDS[i % 5]][i % len(sets[FIELDS[i % 5]])]) for i in range(16)], four


def test_sixteen_requests_in_one_launch_and_the_masks(fx):
    e, m, _ = fx
    s, t = Session(e), Session(e)
    try:
        reqs, four = sixteen(m)
        assert len({r.filter for r in reqs}) == 4 and {r.field for r in reqs} == set(FIELDS)
        got = run(s, m, reqs, "sixteen")
        assert s.last_range_stats() == (4, 0, 1) and s.last_prefilter_stats() == (4, 0, 1)       # four masks in one k_filter_mask_multi launch, one k_range_counts launch
        again = s.range_facets(reqs)
        assert s.last_range_stats() == (0, 4, 1) and again == got
        for r, g in zip(reqs, got):                                                 # every answer equals the same request asked alone
            assert t.range_facets(r.filter, r.field, r.edges) == g
            assert t.last_range_stats()[2] == 1
        assert e.range_facets(reqs) == got                                          # on the engine (its default session)
        assert e.last_range_stats()[2] == 1 and sum(e.last_range_stats()[:2]) == 4
        seventeen = reqs + [RangeRequest(four[0], "uniq", (0, 10, 20))]             # Python splits: 16 + 1
        got17 = run(s, m, seventeen, "seventeen")
        assert len(got17) == 17 and got17[:16] == got and s.last_range_stats() == (0, 1, 1)
        assert e.range_facets(seventeen) == got17
        # no filter: the index's Deleted flags, no mask; three fields of one filter: one mask
        run(s, m, [RangeRequest(None, f, (0, 1000, 2000)) for f in ("shop", "year", "uniq")], "no filter")
        assert s.last_range_stats() == (0, 0, 1)
        run(s, m, [RangeRequest("shop = 41", f, (0, 1000, 2000)) for f in ("shop", "year", "uniq")], "one filter")
        assert s.last_range_stats() == (1, 0, 1)
    finally:
        s.close(); t.close()


def test_refusals_are_per_request(fx):
    e, m, _ = fx
    reqs = [RangeRequest("shop = 31", "year", (1900, 1950, 2000)), RangeRequest("shop = ", "year", (1900, 2000)), RangeRequest("ten MATCHES 'c[12]'", "year", (1900, 2000)),
            RangeRequest("shop = 32", "nosuch", (1, 2)), RangeRequest("shop = 32", "genre", (1, 2)), RangeRequest("shop = 33", "year", (2000, 2000)),
            RangeRequest("shop = 33", "year", (1900.5, 2000.5)), RangeRequest("shop = 33", "rating", (0.0, float("nan"))), RangeRequest("shop = 33", "rating", (-0.0, 0.0)),
            RangeRequest("shop = 33", "year", (1900,)), RangeRequest("nosuch = 3", "rating", (0.0, 5.0, 10.0)), RangeRequest("shop = 34", "uniq", (-5000, 0, 100000))]
    got = e.range_facets(reqs)
    assert got[1].error and "syntax" in got[1].error.lower() and got[1].counts == [] and got[1].total == 0 and got[1].min is None
    assert got[2].error and "MATCHES" in got[2].error
    assert got[3].error and "nosuch" in got[3].error
    assert got[4].error and "string" in got[4].error
    assert got[5].error and "increasing" in got[5].error
    assert got[6].error == "integer column needs integer edges"
    assert got[7].error and "NaN" in got[7].error and got[8].error and "increasing" in got[8].error and got[9].error and "edges" in got[9].error
    for i in (0, 10, 11):
        check(m, got[i], reqs[i])                                                   # an unknown field in the FILTER is null, as the filter VM has it
    assert got[0].total and got[11].total and got[10].total == 0
    assert e.range_facets("shop = ", "year", (1900, 2000)).error == got[1].error
    assert e.range_facets("shop = 31", "year", (1900, 1950, 2000)) == got[0]


def test_deletions_restore_and_a_replaced_column_invalidate(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        sets = {f: edge_sets(m.cols[f][0]) for f in FIELDS}
        reqs = [RangeRequest(EVERYTHING, "year", sets["year"]["at values"]), RangeRequest(ONE_PCT, "rating", sets["rating"]["256 buckets"]), RangeRequest(None, "uniq", sets["uniq"]["between values"]),
                RangeRequest(LAST_ONLY, "shop", (0, 99, 100)), RangeRequest(TWO_COLS, "year", sets["year"]["one bucket"]), RangeRequest(EVERYTHING, "uniq", sets["uniq"]["at values"])]
        before = run(s, m, reqs, "live")
        assert s.range_facets(reqs) == before and s.last_range_stats() == (0, 4, 1)
        top = int(np.argmax(np.asarray(m.cols["uniq"][0])))                         # the document that holds uniq's maximum
        gone = sorted(set(range(0, D, 7)) | {D - 1, top})
        try:
            assert e.delete_documents(gone) == len(gone)
            m.set_deleted(gone)
            got = run(s, m, reqs, "deleted")
            assert s.last_range_stats() == (4, 0, 1)                                # the epoch moved: every mask is built again
            assert got[3].total == 0 and got[3].min is None and got[2].total == D - len(gone) and got[2].max < before[2].max
        finally:
            e.restore_documents(); m.set_deleted([])
        assert run(s, m, reqs, "restored") == before
        # the field's column again, under the same name, with other values (one of them new): thresholds, ranks, masks and min / max follow
        rng = np.random.default_rng(5)
        year = rng.integers(1850, 2031, D).astype(np.int64); year[D - 1] = 2222
        e.set_column("year", year, facetable=True)
        m.cols["year"] = (year, True); m.fm.add_column("year", year, True); m.fm._acc = {}; m.fm._inv = {}
        after = run(s, m, reqs + [RangeRequest("year = 2222", "year", (1850, 2222, 2223)), RangeRequest(None, "year", tuple(range(1850, 2040, 10)))], "replaced column")
        assert s.last_range_stats() == (5, 0, 1)
        assert after[0] != before[0] and after[6].counts == [0, 1] and after[6].max == 2222 and after[7].max == 2222 and after[7].above >= 1
        assert after[5] == before[5]
    finally:
        s.close()
