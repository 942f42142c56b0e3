"""The session's pre-filter masks across the features that read them: list_documents, range_facets and a batch with Query.pre_filter go through one
helper of the engine (filters interned per call, masks found or built in the session's 16 slots, built / reused counted per kind of call), and the tests
of each feature only look at that feature.  Here: one filter's mask built by one feature and reused by the next, the counters of every kind of call after
every other kind, refused requests beside good ones, and the 16-slot least-recently-used rule seen from another feature.

Every listing and every count is also checked against plain numpy on the columns' values: the filters are comparisons on an int and a string column
(evaluated here with numpy), the order of a listing is (rank of the value, document index), the buckets are np.searchsorted(edges, v, side="right").
4 099 documents: 256 groups of 16 and a partial last one of three; three of them deleted."""
import numpy as np
import pytest

from infidex_amd import Document, ListRequest, Query, RangeRequest, SearchEngine
from infidex_amd.engine import Session

pytestmark = pytest.mark.gpu

D = 4099
F = "num < 20"


class Model:
    def __init__(self):
        rng = np.random.default_rng(5)
        self.keys = np.arange(D, dtype=np.int64) * 3 + 1000
        self.num = rng.integers(0, 50, D).astype(np.int64)
        self.val = np.round(rng.normal(0.0, 10.0, D), 1); self.val[rng.integers(0, D, 40)] = np.nan; self.val[D - 1] = 99.5
        self.tag = np.array(["t%d" % (i % 7) for i in range(D)])
        self.live = np.ones(D, bool); self.live[[0, 2048, D - 2]] = False

    def members(self, x):
        """bool per document: live and accepted by filter x (the comparisons the tests use)"""
        acc = {None: np.ones(D, bool), F: self.num < 20, "num >= 30": self.num >= 30, "tag = 't3'": self.tag == "t3",
               "num >= 30 AND tag = 't1'": (self.num >= 30) & (self.tag == "t1")}
        acc.update({"num = %d" % k: self.num == k for k in range(17)})
        return acc[x] & self.live

    def listing(self, r):
        """(document ids, values as text, total) of a ListRequest"""
        idx = np.nonzero(self.members(r.filter))[0]
        key = np.zeros(len(idx), np.int64)
        if r.order_by is not None:
            col = getattr(self, r.order_by)
            v = np.where(np.isnan(col), -np.inf, col) if col.dtype.kind == "f" else col      # NaN is the lowest value
            key = np.unique(v, return_inverse=True)[1][idx]
        page = idx[np.lexsort((idx, key if r.ascending else -key))][r.offset:r.offset + r.limit]
        vals = [] if r.order_by is None else [str(x) for x in getattr(self, r.order_by)[page]]
        return [int(k) for k in self.keys[page]], vals, len(idx)

    def ranges(self, r):
        """(counts, below, above, nan, total, min, max) of a RangeRequest"""
        live = self.members(r.filter)
        v = getattr(self, r.field)[live]
        nan = 0
        if v.dtype.kind == "f":
            nan = int(np.isnan(v).sum()); v = v[~np.isnan(v)]
        c = np.bincount(np.searchsorted(np.asarray(r.edges, v.dtype), v, side="right"), minlength=len(r.edges) + 1)
        cast = float if v.dtype.kind == "f" else int
        return [int(x) for x in c[1:-1]], int(c[0]), int(c[-1]), nan, int(live.sum()), cast(v.min()) if len(v) else None, cast(v.max()) if len(v) else None


@pytest.fixture(scope="module")
def fx():
    m = Model()
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(int(k), "word%d item %d of the shelf" % (i % 11, i)) for i, k in enumerate(m.keys)])
    e.set_column("num", m.num, facetable=True); e.set_column("val", m.val); e.set_column("tag", list(m.tag), facetable=True)
    assert e.delete_documents(m.keys[~m.live]) == 3
    return e, m


def check_listing(m, got, r, values=True):
    ids, vals, total = m.listing(r)
    assert got.error is None, (r, got.error)
    assert (got.document_ids, got.total) == (ids, total), (r, got.document_ids[:8], ids[:8], got.total, total)
    if values and r.order_by != "val":      # (a double's text is ToString()'s, not Python's)
        assert got.values == vals, (r, got.values[:8], vals[:8])


def check_ranges(m, got, r):
    assert got.error is None, (r, got.error)
    assert (got.counts, got.below, got.above, got.nan, got.total, got.min, got.max) == m.ranges(r), (r, got, m.ranges(r))
    assert type(got.min) is type(m.ranges(r)[5])


def test_one_mask_from_feature_to_feature(fx):
    """built by list_documents, reused by range_facets and by a batch's pre-filter; a call without a filter counts nothing"""
    e, m = fx
    s = Session(e)
    try:
        lr = ListRequest(F, "val", False, 5, 300)
        a = s.list_documents(F, "val", False, 5, 300)
        assert s.last_list_stats()[:2] == (1, 0)
        assert s.last_prefilter_stats()[:2] == (1, 0)
        check_listing(m, a, lr)
        rr = RangeRequest(F, "val", (-20.0, -5.0, 0.0, 5.0, 20.0))
        b = s.range_facets(F, "val", rr.edges)
        assert s.last_range_stats() == (0, 1, 1)
        assert s.last_list_stats()[:2] == (1, 0)                         # the listing's counters are the listing's
        check_ranges(m, b, rr)
        res = s.search_queries([Query("item shelf", 10, pre_filter=F), Query("word3", 5, pre_filter=F), Query("word4 item", 5)])
        assert s.last_prefilter_stats()[:2] == (0, 1)
        assert all(r.error is None for r in res)
        assert res[0].total_in_pre_filter == res[1].total_in_pre_filter == a.total == b.total == int(m.members(F).sum()) and res[2].total_in_pre_filter == 0
        accepted = set(int(k) for k in m.keys[m.members(F)])
        assert res[0].records and all(x.document_id in accepted for r in res[:2] for x in r.records)
        lr = ListRequest(None, "num", True, 4000, 200)
        c = s.list_documents(None, "num", True, 4000, 200)
        assert s.last_list_stats()[:2] == (0, 0) and s.last_prefilter_stats() == (0, 0, 0)
        assert s.last_range_stats() == (0, 1, 1)
        check_listing(m, c, lr)
        assert len(c.document_ids) == D - 3 - 4000                       # the partial last group is walked: the page ends with the set
        rr = RangeRequest(None, "num", (0, 10, 25, 49))
        check_ranges(m, s.range_facets(None, "num", rr.edges), rr)
        assert s.last_range_stats() == (0, 0, 1) and s.last_prefilter_stats() == (0, 0, 0)
        assert s.list_documents(F, "val", False, 5, 300) == a and s.last_list_stats()[:2] == (0, 1)
    finally:
        s.close()


def test_refused_requests_beside_good_ones(fx):
    """a syntax error, MATCHES and an unknown field are their request's alone: the good requests of the call answer as a fresh session asked alone"""
    e, m = fx
    s = Session(e)
    try:
        lreqs = [ListRequest("num >= 30", "tag", True, 3, 50), ListRequest("num = ", "num"), ListRequest("tag MATCHES 't[12]'", "num"),
                 ListRequest("tag = 't3'", "nosuch"), ListRequest("num >= 30", "num", False, 0, 1024), ListRequest("num >= 30 AND tag = 't1'", None, True, 1, 7)]
        got = s.list_documents(lreqs)
        assert s.last_list_stats()[:2] == (2, 0)                         # two distinct filters among the good requests
        assert "syntax" in got[1].error.lower() and "MATCHES" in got[2].error and "nosuch" in got[3].error
        assert all((g.document_ids, g.values, g.total) == ([], [], 0) for g in got[1:4])
        rreqs = [RangeRequest("num >= 30", "val", (-10.0, 0.0, 10.0)), RangeRequest("num = ", "num", (0, 10)), RangeRequest("tag MATCHES 't[12]'", "num", (0, 10)),
                 RangeRequest("tag = 't3'", "nosuch", (0, 10)), RangeRequest("tag = 't3'", "num", (5, 6, 7, 40)), RangeRequest("num >= 30", "num", (0, 30, 31, 60))]
        rgot = s.range_facets(rreqs)
        assert s.last_range_stats() == (1, 1, 1)                         # "num >= 30" from the listing, "tag = 't3'" new
        assert "syntax" in rgot[1].error.lower() and "MATCHES" in rgot[2].error and "nosuch" in rgot[3].error
        assert all((g.counts, g.total, g.min, g.max) == ([], 0, None, None) for g in rgot[1:4])
        for i in (0, 4, 5):
            t = Session(e)
            try:
                r = lreqs[i]
                assert t.list_documents(r.filter, r.order_by, r.ascending, r.offset, r.limit) == got[i]
                r = rreqs[i]
                assert t.range_facets(r.filter, r.field, r.edges) == rgot[i]
            finally:
                t.close()
            check_listing(m, got[i], lreqs[i]); check_ranges(m, rgot[i], rreqs[i])
    finally:
        s.close()


def test_sixteen_slots_least_recently_used_across_features(fx):
    """17 distinct filters through list_documents are two device calls; the 17th takes the slot of the first, which range_facets then builds again"""
    e, m = fx
    s = Session(e)
    try:
        reqs = [ListRequest("num = %d" % k, "val", True, 0, 1024) for k in range(17)]
        got = s.list_documents(reqs)
        assert s.last_list_stats()[:2] == (1, 0)                         # of the second call
        for g, r in zip(got, reqs):
            check_listing(m, g, r)
        rr = RangeRequest("num = 0", "num", (0, 1))
        check_ranges(m, s.range_facets(rr.filter, rr.field, rr.edges), rr)
        assert s.last_range_stats() == (1, 0, 1)
        rr = RangeRequest("num = 5", "val", (-100.0, 0.0, 100.0))
        check_ranges(m, s.range_facets(rr.filter, rr.field, rr.edges), rr)
        assert s.last_range_stats() == (0, 1, 1)
    finally:
        s.close()
