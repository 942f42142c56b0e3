"""Browse rows take no boosts, no sort-by and no coverage: SearchEngine.Search returns from HandleEmptyQueryWithFacets (SearchEngine.cs:292-293)
before ApplyPostProcessing.  Browse queries that carry Boosts, SortBy, EnableCoverage and CoverageDepth must equal the model of
tests/browse_model.py exactly — document order and score bits 65535.0f — in per-query form, in session-wide form (set_filter + set_boosts +
set_sort on a Session, which is also what SearchEngine.search(Query) uses), and next to text queries whose rows ARE boosted and sorted."""
import numpy as np
import pytest

from infidex_amd import Query, Boost, BoostStrength
from infidex_amd.engine import Session, pack_texts
from tests.test_gpu_boost_sort import rows_of, assert_rows
from tests.test_gpu_browse import fx, browse, EXPRS, PLACED  # noqa: F401  (fx: that module's fixture, built again for this module)

pytestmark = pytest.mark.gpu

BOOSTS = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low), Boost("rating > 8.0", BoostStrength.Med)]


def decorated(expr, n, sort_by, asc, cov=True, depth=500):
    return Query("", n, filter=expr, enable_facets=True, enable_boost=True, boosts=BOOSTS, sort_by=sort_by, sort_ascending=asc,
                 enable_coverage=cov, coverage_depth=depth)


def test_per_query_boosts_sort_and_coverage_do_not_touch_browse_rows(fx):
    e, o, m, texts = fx
    qs = []
    for i, expr in enumerate([None] + EXPRS + PLACED[:3]):
        qs.append(decorated(expr, [5, 10, 64][i % 3], ["year", "genre", "rating", "nosuchfield"][i % 4], i % 2 == 0, cov=i % 3 != 0, depth=[500, 100][i % 2]))
    text_qs = [Query(texts[i], 10, filter=EXPRS[i], enable_facets=True, enable_boost=True, boosts=BOOSTS, sort_by="year", sort_ascending=True) for i in range(6)]
    mixed = []
    for i, q in enumerate(qs):
        mixed.append(q)
        if i < len(text_qs):
            mixed.append(text_qs[i])
    res = e.search_queries(mixed)
    plain_text = e.search_queries(text_qs)
    undecorated = e.search_queries([browse(q.filter, q.max_number_of_records_to_return) for q in qs])
    bi = ti = 0
    for q, r in zip(mixed, res):
        if q.text == "":
            m.check(r, q.filter, q.max_number_of_records_to_return, ("decorated", q.filter, q.sort_by))
            w = undecorated[bi]; bi += 1
            assert_rows(rows_of(r), rows_of(w), ("same as without boosts / sort", q.filter))
            assert r.facets == w.facets and r.total_in_filter == w.total_in_filter
        else:
            w = plain_text[ti]; ti += 1
            assert_rows(rows_of(r), rows_of(w), ("text", q.text))
            assert r.facets == w.facets
    assert bi == len(qs) and ti == len(text_qs)
    # the text queries next to them were boosted and sorted: their rows differ from the same queries without boosts and sort
    bare = e.search_queries([Query(q.text, 10, filter=q.filter, enable_facets=True) for q in text_qs])
    assert any(rows_of(a) != rows_of(b) for a, b in zip(plain_text, bare))


def test_session_wide_boosts_and_sort_do_not_touch_browse_rows(fx):
    e, o, m, texts = fx
    s = Session(e)
    bits = int(np.float32(65535.0).view(np.uint32))
    try:
        for expr, sort_by, asc in ((EXPRS[0], "year", True), (None, "genre", False), (PLACED[2], "rating", True)):
            s.set_filter(expr, enable_facets=True); s.set_boosts(BOOSTS, True); s.set_sort(sort_by, asc)
            batch = ["", texts[0], "   ", texts[1]]
            arena, offs = pack_texts(batch)
            keys, scores, ties, counts, flags = s.search_packed(arena, offs, 10, 500, True)
            want = m.rows(expr, 10)
            for i in (0, 2):
                assert keys[i, :counts[i]].tolist() == want, (expr, sort_by, keys[i, :counts[i]].tolist(), want)
                assert scores[i, :counts[i]].view(np.uint32).tolist() == [bits] * len(want)
                assert ties[i, :counts[i]].tolist() == [0] * len(want) and int(flags[i]) == 0
                assert e.facets_of(s.h, len(batch), i) == m.row_facets(want)
            per = e.search_queries([Query(t, 10, filter=expr, enable_facets=True, enable_boost=True, boosts=BOOSTS, sort_by=sort_by, sort_ascending=asc) for t in batch])
            for i in (1, 3):                                         # the text queries of the same batch are boosted and sorted as before
                assert keys[i, :counts[i]].tolist() == [x.document_id for x in per[i].records]
                assert scores[i, :counts[i]].view(np.uint32).tolist() == np.asarray([x.score for x in per[i].records], np.float32).view(np.uint32).tolist()
    finally:
        s.set_filter(None, False); s.set_boosts(None, False); s.set_sort(None, False); s.close()
    one = e.search(decorated(EXPRS[1], 10, "year", False))           # SearchEngine.search installs the same session-wide state
    m.check(one, EXPRS[1], 10, "search")
