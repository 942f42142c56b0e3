"""Query.highlight beside the other per-query options on the GPU: the same query with and without `highlight` returns identical records, score bits, ties,
facets, totals and flags — under a filter that drops rows, sort_by, boosts, collapse_by, a pre_filter and max_post_rows=1024 — and the highlights follow the
rows: entry i belongs to record i's document after every reordering, and equals the model's answer (tests/highlight_model.py) for that document.  Refusals
(a browse query, a width out of range) stay per query; a batch without the option reports (0, 0)."""
import dataclasses
import struct

import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength, CoverageSetup
from infidex_amd.engine import Session
from tests import highlight_model as M
from tests.test_gpu_highlight import Texts, assert_highlights

pytestmark = pytest.mark.gpu

N = 400
SHADES = ["red", "green", "golden"]


def build(**kw):
    e = SearchEngine.create_default(device=0, **kw)
    e.index_documents([Document(k, "alpha %s lot %d of the %s harvest" % (SHADES[k % 3], k, ["early", "late"][k % 2])) for k in range(N)])
    k = np.arange(N)
    e.set_column("year", (1950 + (k * 7) % 70).astype(np.int64), facetable=True)
    e.set_column("shade", [SHADES[i % 3] for i in k], facetable=True)
    e.set_column("rank", ((k * 37) % 101).astype(np.int64), facetable=False)
    return e


@pytest.fixture(scope="module")
def engines():
    e, wide = build(), build(max_post_rows=1024, max_depth=1024)
    return (e, Texts(e)), (wide, Texts(wide))


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def same_rows(a, b, ctx):
    assert a.error == b.error, (ctx, a.error, b.error)
    assert [(r.document_id, bits(r.score), r.tiebreaker) for r in a.records] == [(r.document_id, bits(r.score), r.tiebreaker) for r in b.records], ctx
    assert (a.unsupported, a.used_coverage, a.stage1_fallback, a.skipped_candidates) == (b.unsupported, b.used_coverage, b.stage1_fallback, b.skipped_candidates), ctx
    assert a.facets == b.facets and a.total_in_filter == b.total_in_filter and a.total_in_pre_filter == b.total_in_pre_filter, ctx
    assert (a.group_values, a.group_sizes, a.total_groups, a.total_ranked) == (b.group_values, b.group_sizes, b.total_groups, b.total_ranked), ctx
    assert a.pre_filter_facets == b.pre_filter_facets, ctx


BOOSTS = [Boost("year >= 2000", BoostStrength.High), Boost("shade = 'red'", BoostStrength.Low)]
VARIANTS = {
    "plain": dict(),
    "filter": dict(filter="year >= 1990"),
    "filter-facets": dict(filter="year < 1975", enable_facets=True),
    "sort": dict(sort_by="rank", sort_ascending=True),
    "sort-desc-filter": dict(sort_by="year", filter="shade = 'red'"),
    "boosts": dict(enable_boost=True, boosts=BOOSTS),
    "collapse": dict(collapse_by="shade", collapse_keep=3),
    "collapse-sort-filter": dict(collapse_by="year", collapse_keep=1, sort_by="rank", filter="year >= 1960"),
    "pre-filter": dict(pre_filter="year >= 1985", pre_filter_facets=True),
    "everything": dict(pre_filter="year >= 1955", filter="shade = 'golden'", enable_facets=True, enable_boost=True, boosts=BOOSTS, sort_by="rank", collapse_by="shade", collapse_keep=16),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_the_same_rows_with_and_without_highlight(engines, name):
    (e, texts), _ = engines
    base = [Query("alpha golden harvest", 40, **VARIANTS[name]), Query("late lot 7", 25, **VARIANTS[name]), Query("alpa grene", 64, **VARIANTS[name])]
    lit = [dataclasses.replace(q, highlight=True, highlight_chars=24 + 40 * i) for i, q in enumerate(base)]
    without = e.search_queries(base)
    assert e.last_highlight_stats() == (0, 0)
    withh = e.search_queries(lit)
    assert e.last_highlight_stats() == (3, 1)
    rows = 0
    for q, a, b in zip(lit, withh, without):
        same_rows(a, b, (name, q.text))
        assert b.highlights is None
        assert_highlights(q, a, texts, M.Setup(), ctx=name)
        rows += len(a.records)
    assert rows > 0
    # half the batch asks: the others' rows are what they were, and the asking ones' highlights too
    mixed = e.search_queries([lit[0], base[1], lit[2]])
    assert e.last_highlight_stats() == (2, 1)
    for got, want in zip(mixed, [withh[0], without[1], withh[2]]):
        same_rows(got, want, name)
        assert got.highlights == want.highlights


def test_a_thousand_rows_per_query(engines):
    _, (e, texts) = engines
    base = [Query("alpha harvest", 1024, coverage_depth=1024, filter="year >= 1955", sort_by="rank", coverage_setup=CoverageSetup(truncate=False)),
            Query("alpha golden", 300, coverage_depth=1024, sort_by="year", sort_ascending=True)]
    without = e.search_queries(base)
    lit = [dataclasses.replace(q, highlight=True, highlight_chars=32) for q in base]
    withh = e.search_queries(lit)
    assert e.last_highlight_stats() == (2, 1)
    for q, a, b in zip(lit, withh, without):
        same_rows(a, b, q.text)
        assert_highlights(q, a, texts, M.Setup())
    assert len(withh[0].records) > 64


def test_refusals_stay_per_query(engines):
    (e, texts), _ = engines
    qs = [Query("alpha golden", 10, highlight=True), Query("alpha", 10, highlight=True, highlight_chars=15), Query("", 10, enable_facets=True, highlight=True),
          Query("alpha", 10, highlight=True, highlight_chars=513), Query("", 10, enable_facets=True), Query("", 10, highlight=True),
          Query("alpha", 10, collapse_by="nosuch", highlight=True, highlight_chars=0)]
    res = e.search_queries(qs)
    assert e.last_highlight_stats() == (2, 1)                                  # the first and the blank one without facets
    assert_highlights(qs[0], res[0], texts, M.Setup())
    for i in (1, 3):
        assert res[i].records == [] and res[i].highlights is None and "highlight_chars is 16 .. 512" in res[i].error
    assert res[2].records == [] and res[2].highlights is None and "highlight does not apply to a browse query" in res[2].error
    assert res[4].error is None and res[4].records and res[4].highlights is None          # the browse query beside it browses
    assert res[5].error is None and res[5].records == [] and res[5].highlights == []       # an empty text without facets: an empty result, no error
    assert "collapse_by: no field named 'nosuch'" in res[6].error                         # the earlier part's message
    alone = e.search_queries([qs[0]])[0]
    same_rows(alone, res[0], "alone")
    assert alone.highlights == res[0].highlights


def test_a_session_of_its_own(engines):
    (e, texts), _ = engines
    s = Session(e)
    try:
        q = Query("alpha golden", 10, highlight=True, filter="year >= 1990")
        a = s.search_queries([q])[0]
        b = e.search_queries([q])[0]
        same_rows(a, b, "session")
        assert a.highlights == b.highlights
        assert s.search_queries([dataclasses.replace(q, highlight=False)])[0].highlights is None
        assert s.last_highlight_stats() == (0, 0) and e.last_highlight_stats() == (1, 1)
    finally:
        s.close()
