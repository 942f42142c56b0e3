"""Filter, facets, boosts and sort-by on more than 64 returned rows per query (SearchEngine(max_post_rows=...), infx_engine_set_post_rows): the
workgroup-per-query kernels k_postfilter_wide / k_postproc_wide / k_browse_rows_wide next to the one-wave kernels that keep the queries of at most 64 rows.

Expected values follow the convention of tests/test_gpu_boost_sort.py: the base rows of a case are the SAME engine's rows of the same query with no
post-processing (plain parity beyond top-20 is what the parity suites classify); the rows kept by the oracle's filter VM (O.filter_eval), plain counting
for the facets, and tests/bcl_sort.py (held to the host build of the device's wide sort by tests/test_bclsort_wide_model.py) for boosts and sort-by give the
expected keys, tiebreakers and score BITS.  NumberOfDocumentsInFilter is the oracle's; browse rows are tests/browse_model.py's.

The corpus is 1800 short documents with duplicated wording, so hundreds of rows share one score — where the unstable introsort decides the order.  Every case
asserts that its unfiltered base has the number of rows it means to exercise."""
import ctypes as C

import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import InfidexError, Session, pack_texts, _install_query_options
from tests import oracle_lib as O
from tests.browse_model import BrowseModel
from tests.test_gpu_boost_sort import Fixture, columns, rows_of, assert_rows

pytestmark = pytest.mark.gpu

N = 1800
COLOURS = ["red", "green", "golden", "russet", "pink"]
DOCS = [(k, "golden apple orchard harvest %s lot %d" % (COLOURS[k % 5], k)) for k in range(1400)] + \
       [(k, "apple %s pie number %d" % (COLOURS[k % 5], k)) for k in range(1400, N)]
TEXTS = ["golden apple orchard", "apple orchard harvest", "apple"]
SELECTIVE = "year IN (1990, 1991) AND rating > 3.0"   # about thirty of the 1800 documents: a few rows of every base
PERMISSIVE = "year >= 1960 AND genre != 'Horror'"
ALL_PASS = "year >= 1900"
BOOSTS3 = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low), Boost("rating > 8.0", BoostStrength.Med)]
# (rows asked, CoverageDepth, coverage, rows the unfiltered base must have): coverage scores every candidate twice and consolidates, which halves the rows
SHAPES = {65: (65, 500, True), 128: (128, 500, True), 129: (129, 500, True), 250: (250, 500, True),
          256: (256, 500, False), 257: (257, 500, False), 500: (500, 500, False), 1023: (1023, 1024, False), 1024: (1024, 1024, False)}


def make_engine(**kw):
    e = SearchEngine.create_default(device=0, **kw)
    e.index_documents([Document(k, t) for k, t in DOCS])
    return e


class Env:
    def __init__(self):
        self.cols = columns(N)
        year, rating, genre = self.cols
        self.o = O.OracleEngine.create_default(); self.o.index(DOCS)
        self.wide = make_engine(max_post_rows=1024, max_depth=1024)
        self.mid = make_engine(max_post_rows=300)
        self.default = make_engine()
        for x in (self.o, self.wide, self.mid, self.default):
            x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
        self.model = BrowseModel({"year": (year, True), "rating": (rating, False), "genre": (genre, True)})
        self.F = Fixture(self.wide, self.o, self.cols)
        self._base, self._nin = {}, {}

    def base(self, e, k):
        """The engine's own rows of TEXTS with no post-processing, computed once per (engine, shape) and left unchanged."""
        key = (id(e), k)
        if key not in self._base:
            rows, depth, cov = SHAPES[k]
            res = e.search_batch(TEXTS, rows, depth, cov)
            for t, r in zip(TEXTS, res):
                assert len(r.records) == rows, (t, k, len(r.records))
            self._base[key] = [rows_of(r) for r in res]
        return self._base[key]

    def in_filter(self, expr):
        if expr not in self._nin:
            self._nin[expr] = self.o.search_filtered(TEXTS[0], 10, filter=expr, enable_facets=False)["in_filter"]
        return self._nin[expr]

    def expected(self, base, flt, enable_boost, boosts, sort_by, asc):
        kept = [r for r in base if flt is None or self.F.holds(flt, r[0])]
        return kept, self.F.expected(kept, enable_boost, boosts, sort_by, asc)

    def check_result(self, r, base, flt, facets, enable_boost, boosts, sort_by, asc, ctx):
        kept, want = self.expected(base, flt, enable_boost, boosts, sort_by, asc)
        assert_rows(rows_of(r), want, ctx)
        assert r.total_in_filter == (self.in_filter(flt) if flt is not None else 0), ctx
        if facets:
            assert (r.facets or {}) == self.model.row_facets([k for k, _, _ in kept]), ctx
        return kept

    def run(self, e, k, flt=None, facets=False, enable_boost=False, boosts=None, sort_by=None, asc=False):
        rows, depth, cov = SHAPES[k]
        base = self.base(e, k)
        got = e.search_filtered(TEXTS, rows, depth, cov, filter=flt, enable_facets=facets, enable_boost=enable_boost, boosts=boosts, sort_by=sort_by,
                                sort_ascending=asc)
        return [self.check_result(r, b, flt, facets, enable_boost, boosts, sort_by, asc, (t, k, flt, sort_by, asc)) for t, r, b in zip(TEXTS, got, base)]


@pytest.fixture(scope="module")
def env():
    return Env()


def engine_for(env, k):
    return env.mid if k <= 300 and k != 256 else env.wide


@pytest.mark.parametrize("k", sorted(SHAPES))
def test_filter_and_facets(env, k):
    e = engine_for(env, k)
    few = env.run(e, k, flt=SELECTIVE, facets=True)
    assert all(len(x) < k // 8 + 4 for x in few) and (k < 250 or sum(len(x) for x in few) > 0)
    many = env.run(e, k, flt=PERMISSIVE, facets=True)
    assert all(k // 2 < len(x) < k for x in many)
    every = env.run(e, k, flt=ALL_PASS, facets=True)
    assert all(len(x) == k for x in every)
    env.run(e, k, flt=None, facets=True)                         # facets alone


@pytest.mark.parametrize("k", sorted(SHAPES))
def test_boosts_and_sort(env, k):
    e = engine_for(env, k)
    env.run(e, k, flt=PERMISSIVE, facets=True, enable_boost=True, boosts=BOOSTS3, sort_by="rating", asc=k % 2 == 0)
    env.run(e, k, enable_boost=True, boosts=BOOSTS3)
    env.run(e, k, sort_by="genre", asc=k % 2 == 1)


@pytest.mark.parametrize("field", ["year", "rating", "genre", "nosuchfield"])
@pytest.mark.parametrize("ascending", [True, False])
def test_sort_by(env, field, ascending):
    for k in (257, 500):
        env.run(env.wide, k, sort_by=field, asc=ascending)
    env.run(env.wide, 1024, flt=ALL_PASS, sort_by=field, asc=ascending)


def test_equal_scores_really_move(env):
    """Hundreds of equal scores: a boost that matches nothing still re-sorts, and the unstable sort permutes the equal rows."""
    base = env.base(env.wide, 500)
    for b in base:
        sc = [s for _, s, _ in b]
        assert max(sc.count(v) for v in set(sc)) >= 100
    nothing = [Boost("year > 3000", BoostStrength.High)]
    env.run(env.wide, 500, enable_boost=True, boosts=nothing)
    env.run(env.wide, 1024, enable_boost=True, boosts=nothing, sort_by="year", asc=True)
    rows, depth, cov = SHAPES[500]
    moved = env.wide.search_filtered(TEXTS, rows, depth, cov, enable_boost=True, boosts=nothing)
    assert any(rows_of(r) != b and sorted(rows_of(r)) == sorted(b) for r, b in zip(moved, base))


def test_mixed_batch(env):
    """search_queries: narrow and wide post-processing, plain queries beyond 64 rows and one query beyond the engine's post rows in one batch."""
    e = env.wide
    narrow = [Query(TEXTS[0], 20, filter=PERMISSIVE, enable_facets=True, sort_by="year"),
              Query(TEXTS[1], 64, enable_coverage=False, enable_boost=True, boosts=BOOSTS3),
              Query(TEXTS[2], 10, filter=SELECTIVE, enable_facets=True),
              Query(TEXTS[1], 64, enable_coverage=False, filter=ALL_PASS, sort_by="genre", sort_ascending=True)]
    wide = [(500, dict(filter=PERMISSIVE, enable_facets=True, sort_by="rating", sort_ascending=True)),
            (257, dict(enable_boost=True, boosts=BOOSTS3)),
            (250, dict(filter=SELECTIVE, enable_facets=True)),
            (129, dict(enable_facets=True, sort_by="nosuchfield")),
            (500, dict(filter=ALL_PASS, enable_boost=True, boosts=BOOSTS3, sort_by="genre"))]
    wq = [Query(TEXTS[i % 3], SHAPES[k][0], SHAPES[k][1], SHAPES[k][2], **kw) for i, (k, kw) in enumerate(wide)]
    plain = [Query(TEXTS[0], 300, enable_coverage=False), Query(TEXTS[2], 500, enable_coverage=False)]
    refused = Query(TEXTS[1], 1025, enable_coverage=False, filter=PERMISSIVE)
    qs = [narrow[0], wq[0], plain[0], narrow[1], wq[1], refused, wq[2], narrow[2], wq[3], plain[1], narrow[3], wq[4]]
    res = e.search_queries(qs)
    by = {id(q): r for q, r in zip(qs, res)}
    for q, w in zip(narrow, env.default.search_queries(narrow)):     # the one-wave kernels: what an engine that never opted in returns
        r = by[id(q)]
        assert r.error is None and w.error is None
        assert_rows(rows_of(r), rows_of(w), (q.text, q.max_number_of_records_to_return))
        assert r.facets == w.facets and r.total_in_filter == w.total_in_filter
    for i, ((k, kw), q) in enumerate(zip(wide, wq)):
        r = by[id(q)]
        assert r.error is None, r.error
        env.check_result(r, env.base(e, k)[i % 3], kw.get("filter"), kw.get("enable_facets", False), kw.get("enable_boost", False), kw.get("boosts"),
                         kw.get("sort_by"), kw.get("sort_ascending", False), (k, kw))
    for q, n in zip(plain, (300, 500)):
        r = by[id(q)]
        assert r.error is None and len(r.records) == n
        assert_rows(rows_of(r), rows_of(e.search_batch([q.text], n, 500, False)[0]), q.text)
    bad = by[id(refused)]
    assert bad.records == [] and bad.error and "1024" in bad.error, bad.error
    # the raw status and flag bit 4 of the same batch through the C ABI
    s = Session(e)
    status = _install_query_options(e, s.h, qs)
    p = qs.index(refused)
    assert int(status[p]) == 5 and all(int(x) == 0 for i, x in enumerate(status) if i != p)
    arena, offs = pack_texts([q.text for q in qs])
    keys, scores, ties, counts, flags = s.search_packed(arena, offs, 1025, 500, True)
    assert counts[p] == 0 and flags[p] & 16
    assert not any(flags[i] & 16 for i in range(len(qs)) if i != p)
    assert [int(c) for i, c in enumerate(counts) if i != p] == [len(r.records) for i, r in enumerate(res) if i != p]


def test_wide_query_without_facets_has_no_pairs(env):
    """A batch whose only facets belong to a narrow query while its wide query carries just a sort-by or boosts: the wide query's facet pairs, read through
    the C call, are 0 per column — also where the batch before left pairs of a wide query with facets in the same slots."""
    e = env.wide
    s = Session(e)
    rows, depth, cov = SHAPES[500]
    first = [Query(TEXTS[0], rows, depth, cov, enable_facets=True), Query(TEXTS[1], rows, depth, cov, enable_facets=True), Query(TEXTS[1], 20, enable_facets=True)]
    res = s.search_queries(first)
    assert all(r.facets for r in res)
    batch = [Query(TEXTS[0], rows, depth, cov, sort_by="year"), Query(TEXTS[1], rows, depth, cov, enable_boost=True, boosts=BOOSTS3),
             Query(TEXTS[1], 20, enable_facets=True)]
    got = s.search_queries(batch)
    base = env.base(e, 500)
    env.check_result(got[0], base[0], None, False, False, None, "year", False, "sort only")
    env.check_result(got[1], base[1], None, False, True, BOOSTS3, None, False, "boosts only")
    assert got[2].facets == res[2].facets and got[0].facets is None and got[1].facets is None
    L = e.L
    ncol = L.infx_engine_facet_column_count(s.h)
    assert ncol == 2
    codes = np.zeros(128, np.uint32); cnts = np.zeros(128, np.uint32)
    for q in (0, 1):
        for k in range(ncol):
            col = C.c_int32(-1)
            assert L.infx_engine_last_facets(s.h, len(batch), q, k, C.byref(col), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             cnts.ctypes.data_as(C.POINTER(C.c_uint32)), 128) == 0, (q, k)
    col = C.c_int32(-1)
    assert L.infx_engine_last_facets(s.h, len(batch), 2, 0, C.byref(col), codes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     cnts.ctypes.data_as(C.POINTER(C.c_uint32)), 128) > 0


@pytest.mark.parametrize("n", [65, 129, 1024])
def test_browse(env, n):
    e = env.wide
    few, many = "year = 1990", "year >= 1960"
    assert env.model.count(few) < 65 and env.model.count(many) > 1024
    qs = [Query("", n, filter=x, enable_facets=True) for x in (few, many, None)] + [Query("", 10, filter=many, enable_facets=True)]
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        docs = env.model.check(r, q.filter, q.max_number_of_records_to_return, (q.filter, n))
        assert len(docs) == (env.model.count(few) if q.filter == few else q.max_number_of_records_to_return)
        assert r.total_in_filter == (env.in_filter(q.filter) if q.filter is not None else 0)
    for r in e.search_filtered(["", "  "], n, filter=many, enable_facets=True, sort_by="year", enable_boost=True, boosts=BOOSTS3):
        env.model.check(r, many, n, ("search_filtered", n))       # browse rows take no boosts and no sort-by


def test_configured_capacity_is_the_limit(env):
    e = env.mid
    assert e.max_post_rows == 300 and env.wide.max_post_rows == 1024 and env.default.max_post_rows == 64
    ok = e.search_filtered(TEXTS, 300, 500, False, filter=PERMISSIVE, enable_facets=True, sort_by="year")
    base = e.search_batch(TEXTS, 300, 500, False)
    for t, r, b in zip(TEXTS, ok, base):
        assert len(b.records) == 300
        env.check_result(r, rows_of(b), PERMISSIVE, True, False, None, "year", False, (t, 300))
    for kw in (dict(filter=PERMISSIVE), dict(enable_facets=True), dict(enable_boost=True, boosts=BOOSTS3), dict(sort_by="year")):
        with pytest.raises(InfidexError) as ei:
            e.search_filtered(TEXTS, 301, 500, False, **kw)
        assert ei.value.code == 5 and "300" in str(ei.value), (kw, ei.value)
    res = e.search_queries([Query(TEXTS[0], 300, enable_coverage=False, filter=PERMISSIVE), Query(TEXTS[0], 301, enable_coverage=False, filter=PERMISSIVE),
                            Query("", 301, enable_facets=True)])
    assert res[0].error is None and len(res[0].records) == len(ok[0].records)
    assert res[1].records == [] and "300" in res[1].error and res[2].records == [] and "300" in res[2].error
    assert len(e.search_batch(TEXTS, 301, 500, False)[0].records) == 301         # nothing stays installed, plain rows are not limited


def test_default_engine_still_refuses_65_rows(env):
    e = env.default
    for kw in (dict(filter=PERMISSIVE), dict(enable_facets=True), dict(enable_boost=True, boosts=BOOSTS3), dict(sort_by="year")):
        with pytest.raises(InfidexError) as ei:
            e.search_filtered(TEXTS, 65, **kw)
        assert ei.value.code == 5 and "64" in str(ei.value), (kw, ei.value)
    res = e.search_queries([Query(TEXTS[0], 65, filter=PERMISSIVE), Query(TEXTS[0], 64, filter=PERMISSIVE), Query("", 65, enable_facets=True)])
    assert res[0].records == [] and "64" in res[0].error and res[2].records == [] and res[2].error
    assert res[1].error is None and len(res[1].records) > 0


def test_session_wide_setters(env):
    e = env.wide
    rows, depth, cov = SHAPES[257]
    base = env.base(e, 257)
    s = Session(e)
    arena, offs = pack_texts(TEXTS)
    try:
        assert s.set_filter(PERMISSIVE, True) == env.in_filter(PERMISSIVE)
        s.set_boosts(BOOSTS3, True); s.set_sort("genre", True)
        keys, scores, ties, counts, flags = s.search_packed(arena, offs, rows, depth, cov)
        for i, b in enumerate(base):
            c = int(counts[i])
            kept, want = env.expected(b, PERMISSIVE, True, BOOSTS3, "genre", True)
            assert_rows(list(zip(keys[i, :c].tolist(), scores[i, :c].tolist(), ties[i, :c].tolist())), want, TEXTS[i])
            assert (e.facets_of(s.h, len(TEXTS), i) or {}) == env.model.row_facets([k for k, _, _ in kept])
    finally:
        s.set_filter(None, False); s.set_boosts(None, False); s.set_sort(None)
    keys, scores, ties, counts, flags = s.search_packed(arena, offs, rows, depth, cov)
    for i, b in enumerate(base):
        assert_rows(list(zip(keys[i].tolist(), scores[i].tolist(), ties[i].tolist())), b, "cleared")


def test_sharded_equals_unsharded(env):
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards_dev, simulate_set_filter, simulate_set_boosts, simulate_set_sort
    year, rating, genre = env.cols
    W = 3
    engs = [create_sharded_engine(r, W, 0, max_post_rows=300) for r in range(W)]
    for x in engs:
        x.index_documents([Document(k, t) for k, t in DOCS])
        x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
    sess = [ShardSession(x) for x in engs]
    a, off = pack_texts(TEXTS)
    rows, depth, cov = SHAPES[257]
    for flt, sort_by, asc in ((None, "genre", False), (PERMISSIVE, "rating", True)):
        simulate_set_filter(sess, flt, True); simulate_set_boosts(sess, BOOSTS3, True); simulate_set_sort(sess, sort_by, asc)
        res = simulate_shards_dev(sess, a, off, rows, depth, cov)
        for r in res[1:]:
            for x, y in zip(r, res[0]):
                assert np.array_equal(x, y)
        keys, scores, ties, counts, flags = res[0]
        want = env.mid.search_filtered(TEXTS, rows, depth, cov, filter=flt, enable_facets=True, enable_boost=True, boosts=BOOSTS3, sort_by=sort_by, sort_ascending=asc)
        for i, w in enumerate(want):
            c = int(counts[i])
            assert c == len(w.records) and (flt is not None or c == 257)
            assert_rows(list(zip(keys[i, :c].tolist(), scores[i, :c].tolist(), ties[i, :c].tolist())), rows_of(w), (TEXTS[i], flt, sort_by))
            assert (sess[0].facets(i) or {}) == (w.facets or {})
    simulate_set_filter(sess, None, False); simulate_set_boosts(sess, None, False); simulate_set_sort(sess, None)


def test_constructor_and_setter_errors(env):
    for bad in (63, 1025, 0, -1, 2 ** 40):
        with pytest.raises(InfidexError) as ei:
            SearchEngine.create_default(device=0, max_post_rows=bad)
        assert ei.value.code == 1, (bad, ei.value)
    e = make_engine(max_post_rows=64)
    L = e.L
    assert L.infx_engine_set_post_rows(e.h, 128) == 0 and e.max_post_rows == 128      # legal until the first search, indexed or not
    e.search_batch(TEXTS[:1], 10)
    assert L.infx_engine_set_post_rows(e.h, 256) == 1 and e.max_post_rows == 128
    assert b"first search" in C.c_char_p(L.infx_engine_last_error()).value
    e.close()
