"""SearchEngine.facets_of_documents and Query.pre_filter_facets on the GPU: the facets of the documents a filter accepts.

The model is a walk over the documents: the filter decision of a document comes from the oracle's filter VM (BrowseModel.holds, asked once per distinct
combination of the values the expression can read), the rest is plain counting of the accepted live documents' values and the ordering of
tests/browse_model.py.  Every comparison is exact equality of the ordered (value, count) lists and of the totals: the results are integers.

70 001 documents: not a multiple of 4 (the documents of a thread), 64 or 256.  The columns cover the kernel's counter placements (per-workgroup LDS
counters, global counters for the 55 000-value column), the cut at 100 inside a tie, empty values, a facetable column without any value and a
non-facetable one; an int and a double column are there for the filters to read.  Expressions that read one or two columns run with 256 threads per
workgroup, the sixteen of SIXTEEN together read six columns and run with one wave per workgroup."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query
from infidex_amd.engine import Session
from tests.browse_model import BrowseModel, order_facets, facet_text
from tests.test_gpu_boost_sort import rows_of, assert_rows
from tools.synth import Synth

pytestmark = pytest.mark.gpu

D = 70001
ONE_PCT, ON_FACET, NOTHING, EVERYTHING = "shop = 7", "ten = 'c3'", "shop < 0", "shop >= 0"
SIXTEEN = ["shop = 10", "shop = 11", "shop IN (12, 13, 14)", "score > 2.5", "score <= 1.0 AND shop < 50", "ten IN ('c1', 'c2')", "holes = 'h3'",
           "NOT (shop < 90)", "many STARTS WITH 'v19'", "hidden = 'x2' OR shop = 3", "score BETWEEN 1.0 AND 2.0", "shop >= 1", "ten != 'c0' AND score < 4.0",
           "shop = 15 OR shop = 16", "many = 'v100' OR many = 'v229'", "score = 0.5 ? ten = 'c1' : shop = 99"]


def variant(x, depth=1):
    """The same filter under another cache key."""
    return "(" * depth + x + ")" * depth


class FilteredModel:
    """columns as BrowseModel takes them.  accept(): the oracle's filter VM per distinct combination of the values an expression reads; facets():
    plain counting over the accepted documents that are not deleted."""

    def __init__(self, columns, keys=None):
        self.m = BrowseModel(columns, keys)
        self.n = self.m.n
        self.deleted = np.zeros(self.n, bool)
        self._inv = {}
        self._acc = {}

    def add_column(self, name, vals, facetable):
        self.m.columns[name] = (vals, facetable)

    def set_deleted(self, ids):
        self.deleted[:] = False
        self.deleted[list(ids)] = True
        self.m.deleted = set(int(i) for i in ids)

    def inverse(self, name):
        """(number of distinct values, index of each document's value among them)"""
        if name not in self._inv:
            u, inv = np.unique(np.asarray(self.m.columns[name][0]), return_inverse=True)
            self._inv[name] = (len(u), inv.astype(np.int64))
        return self._inv[name]

    def accept(self, expr):
        """bool per document: the filter VM accepts its own fields (Deleted not looked at)"""
        if expr not in self._acc:
            combo = np.zeros(self.n, np.int64)
            for name in [n for n in self.m.columns if n in expr]:
                card, inv = self.inverse(name)
                combo = combo * card + inv
            u, first, inv = np.unique(combo, return_index=True, return_inverse=True)
            table = np.asarray([bool(self.m.holds(expr, int(d))) for d in first])
            self._acc[expr] = table[inv]
        return self._acc[expr]

    def total(self, expr):
        return int((self.accept(expr) & ~self.deleted).sum())

    def facets(self, expr):
        live = self.accept(expr) & ~self.deleted
        out = {}
        for name, (vals, facetable) in self.m.columns.items():
            if not facetable:
                continue
            key = "text:" + name
            if key not in self._inv:
                u, inv = np.unique(np.asarray([facet_text(v) or "" for v in vals]), return_inverse=True)
                self._inv[key] = ([str(x) for x in u], inv.astype(np.int64))
            texts, inv = self._inv[key]
            c = np.bincount(inv[live], minlength=len(texts))
            counts = {t: int(k) for t, k in zip(texts, c) if t and k}
            if counts:
                out[name] = order_facets(counts)
        return out

    def check(self, got, expr, ctx=None):
        assert got.error is None, (ctx, expr, got.error)
        assert got.total == self.total(expr), (ctx, expr, got.total, self.total(expr))
        want = self.facets(expr)
        assert set(got.facets) == set(want), (ctx, expr, sorted(got.facets), sorted(want))
        for name in want:
            assert got.facets[name] == want[name], (ctx, expr, name, got.facets[name][:5], want[name][:5])


@pytest.fixture(scope="module")
def fx():
    s = Synth(2, docs=D)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    rng = np.random.default_rng(11)
    ten = ["c%d" % v for v in rng.integers(0, 10, D)]                              # 10 values
    # 130 values: v100..v189 occur exactly 300 times each (the cut at 100 falls inside a tie), v190..v229 more often
    many = np.concatenate([np.repeat(np.arange(100, 190), 300), rng.integers(190, 230, D - 90 * 300)])
    rng.shuffle(many)
    many = ["v%d" % v for v in many]
    wide = rng.permutation(np.arange(D, dtype=np.int64) % 55000 + 100000)         # 55 000 distinct values: global counters
    holes = [("" if v % 3 == 0 else "h%d" % (v % 7)) for v in rng.integers(0, 1000, D)]   # a third of the documents have no value
    empty = [""] * D                                                               # a facetable field without any value: absent
    hidden = ["x%d" % (v % 5) for v in range(D)]                                   # not facetable
    shop = rng.integers(0, 100, D).astype(np.int64)                                # what the filters read: 100 tenants of about 1 % each
    score = np.round(rng.uniform(0.0, 5.0, D), 1)                                  # 51 doubles
    cols = {"ten": (ten, True), "many": (many, True), "wide": (wide, True), "holes": (holes, True), "empty": (empty, True), "hidden": (hidden, False),
            "shop": (shop, False), "score": (score, False)}
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    qa, qo = s.queries(40, qseed=43, fuzz=0.3)
    return e, FilteredModel(cols), Synth.texts(qa, qo)


def test_single_expressions(fx):
    e, m, _ = fx
    # the vectorised counting of the model is BrowseModel's document-by-document walk
    assert m.facets(EVERYTHING) == m.m.all_facets()
    assert m.total(ONE_PCT) == m.m.count(ONE_PCT) and 500 <= m.total(ONE_PCT) <= 900
    s = Session(e)
    try:
        for x in (ONE_PCT, ON_FACET, NOTHING, EVERYTHING):
            got = s.facets_of_documents(x)
            assert s.last_filtered_facet_stats() == (1, 0, 1), x
            m.check(got, x)
        assert set(s.facets_of_documents(ONE_PCT).facets) == {"ten", "many", "wide", "holes"}
        on = s.facets_of_documents(ON_FACET)
        assert on.facets["ten"] == [("c3", on.total)]                              # the column is read by the filter and counted
        assert s.facets_of_documents(NOTHING) == type(on)({}, 0, None)
        every = s.facets_of_documents(EVERYTHING)
        assert every.facets == e.facets_of_all_documents() and every.total == D
        assert len(every.facets["many"]) == 100 and every.facets["many"][99][1] == 300 and len(every.facets["wide"]) == 100
    finally:
        s.close()


def test_sixteen_in_one_launch_seventeen_in_two_and_the_cache(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        got = s.facets_of_documents(SIXTEEN)
        assert s.last_filtered_facet_stats() == (16, 0, 1)
        for x, g in zip(SIXTEEN, got):
            m.check(g, x, "sixteen")
        assert sum(1 for g in got if g.total) == 16 and len({g.total for g in got}) > 8
        for x, g in zip(SIXTEEN, got):                                             # one by one: other launch shapes and counter placements, same sums
            alone = s.facets_of_documents(variant(x))
            assert s.last_filtered_facet_stats() == (1, 0, 1), x
            assert alone == g, x
        seventeen = [variant(x, 2) for x in SIXTEEN] + ["shop = 42"]
        more = s.facets_of_documents(seventeen)
        assert s.last_filtered_facet_stats() == (17, 0, 2)
        assert more[:16] == got
        m.check(more[16], "shop = 42")
        again = s.facets_of_documents(seventeen)                                   # everything from the cache: nothing is launched
        assert s.last_filtered_facet_stats() == (0, 17, 0)
        assert again == more
        t = Session(e)                                                             # the cache is the engine's: another session finds the answers
        try:
            assert t.facets_of_documents(seventeen) == more and t.last_filtered_facet_stats() == (0, 17, 0)
            mixed = t.facets_of_documents(["shop = 42", "shop = 43", "shop = 42"])   # a repeated expression is counted once
            assert t.last_filtered_facet_stats() == (1, 1, 1) and mixed[0] == mixed[2] == more[16]
            m.check(mixed[1], "shop = 43")
        finally:
            t.close()
    finally:
        s.close()


def small_engine(n, cols):
    s = Synth(2, docs=n)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    return e, FilteredModel(cols)


def test_lds_budget_a_column_goes_to_global_counters():
    """Five columns of 4000 values and one of 3.  One program: four of the large columns fit the 16 384 words of LDS counters beside the small one,
    the fifth counts in global memory.  Sixteen programs in one launch: 16 x 4000 words fit for none of them, all five count in global memory, the
    small column (48 words) stays in LDS.  Integer sums do not depend on the placement: both equal the model and each other."""
    n = 30000
    rng = np.random.default_rng(17)
    cols = {}
    for k in range(5):
        cols["f%d" % k] = (["w%04d" % v for v in rng.integers(0, 4000, n)], True)
    cols["tiny"] = (["t%d" % v for v in rng.integers(0, 3, n)], True)
    cols["shop"] = (rng.integers(0, 32, n).astype(np.int64), False)
    e, m = small_engine(n, cols)
    exprs = ["shop = %d" % i for i in range(12)] + ["shop >= 16", "tiny = 't1'", "shop >= 0", "tiny != 't0' AND shop < 8"]
    one = [e.facets_of_documents(variant(x)) for x in exprs]
    assert e.last_filtered_facet_stats() == (1, 0, 1)
    got = e.facets_of_documents(exprs)
    assert e.last_filtered_facet_stats() == (16, 0, 1)
    assert got == one
    for x, g in zip(exprs, got):
        m.check(g, x)
    assert all(len(got[14].facets["f%d" % k]) == 100 for k in range(5)) and got[14].total == n
    gone = list(range(5, n, 11))
    assert e.delete_documents(gone) == len(gone)
    m.set_deleted(gone)
    got = e.facets_of_documents(exprs)
    assert e.last_filtered_facet_stats() == (16, 0, 1)
    for x, g in zip(exprs, got):
        m.check(g, x, "deleted")


def test_lds_budget_fewer_programs_per_launch():
    """Five columns of 250 values: columns this small always count in LDS, and sixteen programs x 1250 words exceed the 16 384 words, so the call is
    split evenly into two launches of eight programs.  Same answers as one program per launch."""
    n = 9001
    rng = np.random.default_rng(23)
    cols = {}
    for k in range(5):
        cols["g%d" % k] = (["u%03d" % v for v in rng.integers(0, 250, n)], True)
    cols["shop"] = (rng.integers(0, 20, n).astype(np.int64), False)
    e, m = small_engine(n, cols)
    exprs = ["shop = %d" % i for i in range(14)] + ["shop >= 0", "g0 STARTS WITH 'u00'"]
    got = e.facets_of_documents(exprs)
    assert e.last_filtered_facet_stats() == (16, 0, 2)
    for x, g in zip(exprs, got):
        m.check(g, x)
        assert e.facets_of_documents(variant(x)) == g and e.last_filtered_facet_stats() == (1, 0, 1), x
    assert e.facets_of_documents(exprs[:8]) == got[:8] and e.last_filtered_facet_stats() == (0, 8, 0)


def test_totals_are_the_pre_filter_counts(fx):
    e, m, texts = fx
    s = Session(e)
    try:
        for x in (ONE_PCT, ON_FACET, NOTHING, "score > 2.5 AND shop < 50"):
            total = s.facets_of_documents(x).total
            assert total == int((s.prefilter_mask(x) == 0).sum()), x
            r = s.search_queries([Query(texts[0], 10, pre_filter=x)])[0]
            assert r.error is None and total == r.total_in_pre_filter, x
    finally:
        s.close()


def test_duplicate_keys_count_each_document_by_its_own_fields():
    """Several documents per key, one of them deleted on its own: a document counts when IT is live and ITS fields pass, whatever the key's first live
    document looks like — as total_in_pre_filter and the masks."""
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    keys = [10, 11, 10, 12, 11, 10, 13, 12, 14, 13, 14, 15]           # key 10: documents 0, 2, 5; key 11: 1, 4; ...
    shade = ["red", "blue", "blue", "red", "red", "green", "blue", "blue", "green", "green", "red", "blue"]
    size = np.asarray([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(k, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i, k in enumerate(keys)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    m = FilteredModel({"shade": (shade, True), "size": (size, False)}, keys)
    exprs = ["shade = 'red'", "shade = 'blue'", "size >= 6", "shade != 'green' AND size < 9", "size >= 0"]
    for deleted in ([], [0, 7]):                                       # document 0: the first of key 10; 7: the second of key 12
        if deleted:
            assert e.delete_document_ids(deleted) == len(deleted)
            m.set_deleted(deleted)
        got = e.facets_of_documents(exprs)
        for x, g in zip(exprs, got):
            m.check(g, x, deleted)
            assert g.total == int((e.prefilter_mask(x) == 0).sum()), (x, deleted)
            r = e.search_queries([Query("alpha", 10, pre_filter=x)])[0]
            assert r.error is None and r.total_in_pre_filter == g.total, (x, deleted)
    assert got[0].facets == {"shade": [("red", 3)]} and got[4].total == 10


def test_search_queries_with_pre_filter_facets(fx):
    e, m, texts = fx
    tenants = ["shop = 21", "shop = 22", "shop = 23"]

    def batch(flag):
        qs = []
        for i, t in enumerate(texts[:12]):
            pre = tenants[i % 4] if i % 4 < 3 else None                # every fourth query is a plain one
            qs.append(Query(t, [5, 10, 20][i % 3], pre_filter=pre, pre_filter_facets=flag and (pre is None or i != 1), enable_facets=(i % 2 == 0),
                            filter="score > 1.0" if i % 5 == 0 else None))
        qs.append(Query("", 10, enable_facets=True, pre_filter_facets=flag))      # a browse query: no pre-filter, nothing to count
        return qs
    s = Session(e)
    try:
        plain = s.search_queries(batch(False))
        assert s.last_filtered_facet_stats() == (0, 0, 0)
        got = s.search_queries(batch(True))
        assert s.last_filtered_facet_stats() == (3, 0, 1)              # the three tenants in one launch
        want = dict(zip(tenants, e.facets_of_documents(tenants)))
        for i, (q, r, w) in enumerate(zip(batch(True), got, plain)):
            assert r.error is None and w.error is None
            assert_rows(rows_of(r), rows_of(w), i)
            assert (r.facets, r.total_in_filter, r.total_in_pre_filter) == (w.facets, w.total_in_filter, w.total_in_pre_filter), i
            assert w.pre_filter_facets is None
            if q.pre_filter is not None and q.pre_filter_facets:
                assert r.pre_filter_facets == want[q.pre_filter].facets == m.facets(q.pre_filter), i
                assert r.total_in_pre_filter == want[q.pre_filter].total
            else:
                assert r.pre_filter_facets is None, i
        assert got[1].pre_filter_facets is None and got[1].total_in_pre_filter == m.total(tenants[1])      # it has a pre-filter but did not ask
        assert got[12].records and got[12].facets
        s.search_queries(batch(True))                                  # the same tenants again: nothing is counted
        assert s.last_filtered_facet_stats() == (0, 3, 0)
        one = e.search(Query(texts[0], 10, pre_filter=tenants[0], pre_filter_facets=True))
        assert one.pre_filter_facets == want[tenants[0]].facets
        # a refused pre-filter keeps its error and gets no facets
        bad = s.search_queries([Query(texts[0], 10, pre_filter="shop = ", pre_filter_facets=True), Query(texts[1], 10, pre_filter=tenants[0], pre_filter_facets=True)])
        assert bad[0].error and bad[0].pre_filter_facets is None and bad[0].records == []
        assert bad[1].error is None and bad[1].pre_filter_facets == want[tenants[0]].facets
    finally:
        s.close()


def test_two_runs_and_two_sessions_agree(fx):
    e, m, _ = fx
    exprs = [EVERYTHING, "score > 2.5", "ten IN ('c1', 'c2')", "wide >= 140000"]
    s = Session(e)
    try:
        a = e.facets_of_documents([variant(x, 3) for x in exprs])
        assert e.last_filtered_facet_stats() == (4, 0, 1)
        b = s.facets_of_documents([variant(x, 4) for x in exprs])
        assert s.last_filtered_facet_stats() == (4, 0, 1)
        c = s.facets_of_documents([variant(x, 5) for x in exprs])
        assert a == b == c
        m.check(a[3], exprs[3])
    finally:
        s.close()


def test_refusals_are_per_expression(fx):
    e, m, _ = fx
    exprs = ["shop = 31", "shop = ", "ten MATCHES 'c[12]'", "nosuch = 3", "nosuch IS NULL AND shop = 32", "shop = 33"]
    got = e.facets_of_documents(exprs)
    assert e.last_filtered_facet_stats() == (4, 0, 1)
    assert got[1].error and "syntax" in got[1].error.lower() and got[1].facets == {} and got[1].total == 0
    assert got[2].error and "MATCHES" in got[2].error and got[2].facets == {} and got[2].total == 0
    for i in (0, 3, 4, 5):
        m.check(got[i], exprs[i])                                      # an unknown field is null, as the filter VM has it
    assert got[0].total and got[5].total
    single = e.facets_of_documents("shop = ")
    assert single.error == got[1].error


def test_deletions_restore_and_a_new_column_invalidate_the_cache(fx):
    e, m, _ = fx
    exprs = [ONE_PCT, ON_FACET, EVERYTHING, "score > 2.5"]
    s = Session(e)
    try:
        before = s.facets_of_documents(exprs)
        assert s.facets_of_documents(exprs) == before and s.last_filtered_facet_stats() == (0, 4, 0)
        gone = sorted(set(range(0, D, 7)) | {D - 1})
        try:
            assert e.delete_documents(gone) == len(gone)
            m.set_deleted(gone)
            got = s.facets_of_documents(exprs)
            assert s.last_filtered_facet_stats() == (4, 0, 1)
            for x, g in zip(exprs, got):
                m.check(g, x, "deleted")
            assert got[2].total == D - len(gone) and got[2].facets == e.facets_of_all_documents()
        finally:
            e.restore_documents(); m.set_deleted([])
        got = s.facets_of_documents(exprs)
        assert s.last_filtered_facet_stats() == (4, 0, 1) and got == before
        extra = ["e%d" % (d % 13) for d in range(D)]
        e.set_column("extra", extra, facetable=True); m.add_column("extra", extra, True)
        got = s.facets_of_documents(exprs + ["extra = 'e5' AND shop < 50"])
        assert s.last_filtered_facet_stats() == (5, 0, 1)
        for x, g in zip(exprs + ["extra = 'e5' AND shop < 50"], got):
            m.check(g, x, "new column")
            assert "extra" in g.facets
    finally:
        s.close()
