"""Browse queries on the GPU: empty text + EnableFacets (SearchEngine.HandleEmptyQueryWithFacets, SearchEngine.cs:321-346) — the first
MaxNumberOfRecordsToReturn live documents in index order that pass Query.Filter, score 65535, plus the facets of those rows.

Expected values come from tests/browse_model.py (a walk over the documents with the oracle's filter VM), NumberOfDocumentsInFilter from
OracleEngine.search_filtered(...)["in_filter"]; every comparison is exact.  The corpus has more than 65 536 documents so the ordered scan crosses
that boundary; `pos` is the document index, which lets a filter place its first matches anywhere."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import Session
from tests import oracle_lib as O
from tests.browse_model import BrowseModel
from tests.test_gpu_boost_sort import columns, rows_of, assert_rows
from tools.synth import Synth

pytestmark = pytest.mark.gpu

D = 70000
EXPRS = ["year >= 2000 AND rating > 7.0", "genre IN ('Drama', 'crime') OR year < 1960", "NOT (rating <= 5) AND genre != 'Horror'",
         "year BETWEEN 1990 AND 1999", "genre STARTS WITH 'S' OR genre LIKE '%er'", "rating >= 9.5 ? genre = 'Action' : year >= 2020",
         "rating = 7", "nosuchfield IS NULL AND year > 2010", "genre IN ('Comedy', 'Western', 'Fantasy')", "year < 1980",
         "rating > 5.5 AND rating < 8.5", "nosuchfield = 'x' OR genre = 'Drama'"]
PLACED = ["pos >= %d" % (D - 10), "pos BETWEEN 250 AND 260", "pos IN (0, 255, 256, 65535, 65536)", "pos = %d" % (D - 1), "pos > %d" % D,
          "pos IN (3, 40000, 69000)"]


@pytest.fixture(scope="module")
def fx():
    s = Synth(2, docs=D)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    year, rating, genre = columns(D)
    pos = np.arange(D, dtype=np.int64)
    for x in (e, o):
        x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
        x.set_column("pos", pos, facetable=False)
    m = BrowseModel({"year": (year, True), "rating": (rating, False), "genre": (genre, True), "pos": (pos, False)})
    qa, qo = s.queries(40, qseed=43, fuzz=0.3)
    return e, o, m, Synth.texts(qa, qo)


def browse(expr, n):
    return Query("", n, filter=expr, enable_facets=True)


def in_filter(o, text, expr):
    return o.search_filtered(text, 10, filter=expr, enable_facets=False)["in_filter"]


def test_first_rows_of_each_filter(fx):
    e, o, m, texts = fx
    qs = [browse(x, n) for x in [None] + EXPRS for n in (1, 5, 10, 64)]
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        docs = m.check(r, q.filter, q.max_number_of_records_to_return, (q.filter, q.max_number_of_records_to_return))
        assert len(docs) == q.max_number_of_records_to_return
        assert r.total_in_filter == (in_filter(o, texts[0], q.filter) if q.filter is not None else 0), q.filter
    one = e.search(browse(EXPRS[0], 10))                             # SearchEngine.search and search_filtered take the same branch
    m.check(one, EXPRS[0], 10, "search")
    many = e.search_filtered(["", "  "], 10, filter=EXPRS[1], enable_facets=True)
    for r in many:
        m.check(r, EXPRS[1], 10, "search_filtered")


def test_matches_placed_where_a_scan_goes_wrong(fx):
    e, o, m, texts = fx
    qs = [browse(x, n) for x in PLACED for n in (1, 10, 64)]
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        m.check(r, q.filter, q.max_number_of_records_to_return, (q.filter, q.max_number_of_records_to_return))
        assert r.total_in_filter == in_filter(o, texts[0], q.filter), q.filter
    by = {(q.filter, q.max_number_of_records_to_return): r for q, r in zip(qs, res)}
    assert [x.document_id for x in by[(PLACED[0], 64)].records] == list(range(D - 10, D))              # fewer matches than asked
    assert [x.document_id for x in by[(PLACED[2], 10)].records] == [0, 255, 256, 65535, 65536]
    assert [x.document_id for x in by[(PLACED[3], 10)].records] == [D - 1]                             # one match, in the last document
    none = by[(PLACED[4], 10)]
    assert none.records == [] and (none.facets or {}) == {} and none.total_in_filter == 0             # no match at all


def test_deleted_documents_are_skipped_and_return_after_restore(fx):
    e, o, m, texts = fx
    gone = [0, 1, 5, 255, 256, 65536, D - 1]
    qs = [browse(None, 10), browse(PLACED[2], 10), browse(PLACED[3], 5), browse(EXPRS[3], 64)]
    try:
        assert e.delete_documents(gone) == len(gone)
        o.delete_keys(gone); m.deleted = set(gone)
        res = e.search_queries(qs)
        for q, r in zip(qs, res):
            m.check(r, q.filter, q.max_number_of_records_to_return, ("deleted", q.filter))
            if q.filter is not None:
                assert r.total_in_filter == in_filter(o, texts[0], q.filter), q.filter
        assert [x.document_id for x in res[0].records] == [2, 3, 4, 6, 7, 8, 9, 10, 11, 12]
        assert [x.document_id for x in res[1].records] == [65535] and res[1].total_in_filter == 1
        assert res[2].records == [] and res[2].total_in_filter == 0
    finally:
        e.restore_documents(); o.restore_all(); m.deleted = set()
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        m.check(r, q.filter, q.max_number_of_records_to_return, ("restored", q.filter))
    assert [x.document_id for x in res[1].records] == [0, 255, 256, 65535, 65536] and res[1].total_in_filter == 5


def test_blank_without_facets_stays_empty_and_too_many_rows_are_refused(fx):
    e, o, m, texts = fx
    qs = [Query("", 10), Query("   ", 10), Query("", 10, filter=EXPRS[0]), browse(EXPRS[0], 5), browse(None, 100), browse(EXPRS[1], 7), Query("   ", 3, enable_facets=True)]
    res = e.search_queries(qs)
    for r in res[:3]:
        assert r.records == [] and r.error is None and r.facets is None
        assert (r.unsupported, r.used_coverage, r.stage1_fallback, r.skipped_candidates) == (False, False, False, False)
    m.check(res[3], EXPRS[0], 5); m.check(res[5], EXPRS[1], 7); m.check(res[6], None, 3)
    assert res[4].records == [] and res[4].error                      # facets run on at most 64 rows: refused on its own
    s = Session(e)
    from infidex_amd.engine import _install_query_options
    status = _install_query_options(e, s.h, qs)
    assert status.tolist() == [0, 0, 0, 0, 5, 0, 0]                   # INFX_EUNSUPPORTED
    e.L.infx_engine_set_query_options(s.h, 0, None, None)
    s.close()
    assert e.search_batch(["", "  "], 10)[0].records == []


def test_mixed_batch_with_text_queries_and_300_expressions(fx):
    e, o, m, texts = fx
    rng = np.random.default_rng(3)
    boosts = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low)]
    text_qs = []
    for i in range(48):
        text_qs.append(Query(texts[i % len(texts)], int(rng.choice([5, 10, 20])), filter=None if i % 4 == 0 else EXPRS[i % len(EXPRS)], enable_facets=i % 2 == 0,
                             enable_boost=i % 3 == 0, boosts=boosts if i % 3 == 0 else None, sort_by=[None, "year", "genre"][i % 3], sort_ascending=i % 2 == 1))
    exprs = ["pos >= %d AND year >= %d" % (7 * i if i % 50 else 260 * i, 1950 + i % 40) for i in range(300)] + EXPRS      # a few start far into the corpus
    browse_qs = [browse(x, int(rng.choice([1, 3, 10, 64]))) for x in exprs] + [browse(None, 10), browse(exprs[5], 64)]
    assert len(set(q.filter for q in browse_qs if q.filter)) >= 300
    mixed, where = [], []
    ti = bi = 0
    while ti < len(text_qs) or bi < len(browse_qs):                   # interleaved: a text query after every seventh browse query
        if bi < len(browse_qs) and (ti >= len(text_qs) or (bi + 1) % 7):
            mixed.append(browse_qs[bi]); where.append(("b", bi)); bi += 1
        else:
            mixed.append(text_qs[ti]); where.append(("t", ti)); ti += 1
    e.search_queries([browse(x, 1) for x in EXPRS])                    # every one of EXPRS has its count cached from here on
    plain = e.search_queries(text_qs)
    res = e.search_queries(mixed)
    counted, launches = e.last_count_stats()
    assert (counted, launches) == (300, 0)                            # the scan counted the 300 expressions the batch saw first
    assert e.last_browse_stats() == (313, 2)                          # 300 + EXPRS + "no filter" groups: more than 256, so two scan launches
    assert any(r.records for r in plain)
    for (kind, i), r in zip(where, res):
        if kind == "t":
            w = plain[i]
            assert r.error is None and w.error is None
            assert_rows(rows_of(r), rows_of(w), ("text", i))
            assert (r.unsupported, r.used_coverage, r.stage1_fallback, r.skipped_candidates) == (w.unsupported, w.used_coverage, w.stage1_fallback, w.skipped_candidates)
            assert r.total_in_filter == w.total_in_filter and r.facets == w.facets, ("text", i)
        else:
            q = browse_qs[i]
            m.check(r, q.filter, q.max_number_of_records_to_return, ("browse", i, q.filter))
    for i in (0, 17, 150, 299, 305):                                  # counts of a sample against the oracle
        q = browse_qs[i]
        r = res[where.index(("b", i))]
        assert r.total_in_filter == in_filter(o, texts[0], q.filter), q.filter


def test_expression_first_seen_in_a_browse_query_is_counted_by_the_scan(fx):
    e, o, m, texts = fx
    expr = "year >= 1987 AND pos >= 1234 AND rating < 9.9"
    r = e.search_queries([browse(expr, 10)])[0]
    want = in_filter(o, texts[0], expr)
    m.check(r, expr, 10)
    assert r.total_in_filter == want and want > 0
    assert e.last_count_stats() == (1, 0)                             # counted, with no k_filter_count_multi launch
    t = e.search_queries([Query(texts[0], 10, filter=expr)])[0]
    assert t.total_in_filter == want
    assert e.last_count_stats() == (0, 0)                             # served from the cache
    again = e.search_queries([browse(expr, 10)])[0]                   # cached count + rows only
    m.check(again, expr, 10)
    assert again.total_in_filter == want and e.last_count_stats() == (0, 0)


def test_session_wide_path_gives_the_same_rows(fx):
    e, o, m, texts = fx
    s = Session(e)
    try:
        for expr in (None, EXPRS[0], PLACED[2]):
            nin = s.set_filter(expr, enable_facets=True)
            batch = [texts[0], "", texts[1], "   ", ""]
            from infidex_amd.engine import pack_texts
            arena, offs = pack_texts(batch)
            keys, scores, ties, counts, flags = s.search_packed(arena, offs, 10, 500, True)
            per = e.search_queries([Query(t, 10, filter=expr, enable_facets=True) for t in batch])
            want = m.rows(expr, 10)
            for i, t in enumerate(batch):
                assert keys[i, :counts[i]].tolist() == [x.document_id for x in per[i].records], (expr, i)
                assert scores[i, :counts[i]].view(np.uint32).tolist() == np.asarray([x.score for x in per[i].records], np.float32).view(np.uint32).tolist()
                assert e.facets_of(s.h, len(batch), i) == (per[i].facets or {}), (expr, i)
                if not t.strip():
                    assert keys[i, :counts[i]].tolist() == want and int(flags[i]) == 0
            if expr is not None:
                assert nin == in_filter(o, texts[0], expr)
    finally:
        s.set_filter(None, False); s.close()


def test_two_runs_return_identical_arrays(fx):
    e, o, m, texts = fx
    qs = [browse(x, 64) for x in EXPRS + PLACED + [None]] + [Query(texts[i], 10, filter=EXPRS[i], enable_facets=True) for i in range(6)]
    a = e.search_queries(qs); b = e.search_queries(qs)
    for x, y in zip(a, b):
        assert rows_of(x) == rows_of(y) and x.facets == y.facets and x.total_in_filter == y.total_in_filter
        assert np.asarray([r.score for r in x.records], np.float32).tobytes() == np.asarray([r.score for r in y.records], np.float32).tobytes()


def test_duplicate_keys_rows_per_document_filter_by_first_live_document():
    """Several documents per key: one row per live document; the filter (and the facets) look at the key's first live document, the count at each
    live document's own fields (ResultProcessor.cs:39-54, 58-66; DocumentCollection.cs:60-82)."""
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    keys = [10, 11, 10, 12, 11, 10, 13, 12, 14, 13, 14, 15]           # key 10: documents 0, 2, 5; key 11: 1, 4; ...
    shade = ["red", "blue", "blue", "red", "red", "green", "blue", "blue", "green", "green", "red", "blue"]
    size = np.asarray([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(k, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i, k in enumerate(keys)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    m = BrowseModel({"shade": (shade, True), "size": (size, False)}, keys)
    exprs = [None, "shade = 'red'", "shade = 'blue'", "size >= 6", "shade != 'green' AND size < 9"]

    def run(tag):
        res = e.search_queries([browse(x, n) for x in exprs for n in (3, 12)])
        it = iter(res)
        for x in exprs:
            for n in (3, 12):
                r = next(it)
                m.check(r, x, n, (tag, x, n))
                if x is not None:
                    assert r.total_in_filter == m.count(x), (tag, x, r.total_in_filter)
        return {x: [d for d in m.rows(x, 12)] for x in exprs}

    before = run("all live")
    assert before["shade = 'red'"] == [0, 2, 3, 5, 7]                 # keys 10 and 12: decided by documents 0 and 3, whatever the rows' own shade
    assert len(before[None]) == 12                                    # one row per document, not per key
    assert e.delete_document_ids([0]) == 1                            # key 10's first live document becomes 2 (blue)
    m.deleted = {0}
    during = run("first document of key 10 deleted")
    assert during["shade = 'red'"] == [3, 7] and during["shade = 'blue'"] == [1, 2, 4, 5, 6, 9, 11]
    e.restore_documents(); m.deleted = set()
    assert run("restored") == before
    assert e.delete_documents([12]) == 2                              # by key: every document of key 12
    m.deleted = {3, 7}
    assert run("key 12 deleted")["shade = 'red'"] == [0, 2, 5]
    e.restore_documents()
