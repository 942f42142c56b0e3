"""Facets of list columns on the GPU: facets_of_all_documents, facets_of_documents and Query.pre_filter_facets count the element occurrences of every
value of a facetable list column among the live documents (the filter accepts) — a duplicate counts twice, an empty string never, a deleted document's
elements never — ordered and cut as the scalar facets, which stay what they are without any list column.  Result.facets (the returned rows, a browse
query) has no list-column key.

The model is tests/list_column_model.py (a collections.Counter over elements); the corpus is tests/test_gpu_list_columns.py's: the 33-value and 32-value
columns count in per-workgroup LDS, the column one above k_list_leaf's bitmap budget (65 537 values) in global memory — K x V against 16 384 words
decides.  The module's expressions hold fifteen distinct list-column leaves in all: within the engine's sixteen derived columns.  Every comparison is exact."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Query
from infidex_amd.engine import Session
from tests import list_column_model as M
from tests.test_gpu_boost_sort import rows_of, assert_rows
from tests.test_gpu_list_columns import BIG, L, documents, make_engine

pytestmark = pytest.mark.gpu

GENRES = ["drama", "comedy", "noir"]
SIXTEEN = [L("tags", "=", "t31"), L("tags", "IS NULL"), L("v32", "<", 3), L("big", "<", 64), ("not", L("tags", "=", "t05")), ("scalar", "year", "=", 2003),
           ("and", L("tags", "STARTS WITH", "t1"), ("scalar", "year", ">=", 2004)), ("or", L("v32", "=", 7), L("tags", "=", "")), L("none", "IS NULL"),
           L("none", "=", "x"), L("v32", "IN", 1, 2, 31), L("tags", "CONTAINS", "3"), ("scalar", "year", "<", 2002), L("v32", "BETWEEN", 10, 12),
           L("big", "=", BIG - 1), ("not", L("none", "IS NULL"))]


def set_scalars(e):
    e.set_column("genre", [GENRES[(d * 5) % 3] for d in range(M.N)], facetable=True)


@pytest.fixture(scope="module")
def fx():
    columns = M.corpus(BIG)
    e = make_engine(columns); set_scalars(e)
    plain = SearchEngine.create_default(device=0)                        # the same corpus without any list column
    plain.index_documents(documents())
    plain.set_column("year", np.asarray([M.year_of(d) for d in range(M.N)], np.int64), facetable=True); set_scalars(plain)
    for x in (e, plain):
        assert x.delete_document_ids(M.DELETED) == len(M.DELETED)
    yield e, plain, columns
    e.close(); plain.close()


def live():
    return [d for d in range(M.N) if d not in M.DELETED]


def test_facets_of_all_documents(fx):
    e, plain, columns = fx
    got, scalar = e.facets_of_all_documents(), plain.facets_of_all_documents()
    want = M.facets(columns, live())
    assert set(want) == {"tags", "v32", "big"} and set(scalar) == {"year", "genre"}      # `none` has no value: absent
    assert {k: v for k, v in got.items() if k in scalar} == scalar
    assert {k: v for k, v in got.items() if k not in scalar} == want
    assert len(got["big"]) == 100 and len(got["tags"]) == 32 and all(v != "" for v, _ in got["tags"])      # cut at 100; the empty string is no value


def test_duplicates_count_twice_and_deleted_documents_not_at_all(fx):
    e, _, columns = fx
    tags = columns["tags"][0]
    got = dict(e.facets_of_all_documents()["tags"])
    assert got["t05"] == sum(l.count("t05") for d, l in enumerate(tags) if d not in M.DELETED)
    assert got["t05"] >= 5 + sum(1 for d, l in enumerate(tags) if "t05" in l and d not in M.DELETED and d != M.DUPLICATES)       # the five of one document
    dead = [d for d in M.DELETED if tags[d]]
    assert dead and sum(got.values()) == sum(len([x for x in l if x != ""]) for d, l in enumerate(tags) if d not in M.DELETED)
    only = e.facets_of_documents("tags = 't05' AND year = %d" % M.year_of(M.DUPLICATES))
    docs = [d for d in live() if "t05" in tags[d] and M.year_of(d) == M.year_of(M.DUPLICATES)]
    assert M.DUPLICATES in docs and only.total == len(docs)             # total counts documents, the facet counts elements
    assert dict(only.facets["tags"])["t05"] == sum(tags[d].count("t05") for d in docs) > len(docs)


def test_facets_of_sixteen_expressions_in_one_call(fx):
    e, plain, columns = fx
    s = Session(e)
    try:
        exprs = [M.text(x) for x in SIXTEEN]
        got = s.facets_of_documents(exprs)
        scalar = plain.facets_of_documents([M.text(x) for x in SIXTEEN if "scalar" == x[0]])
        assert s.last_filtered_facet_stats()[:2] == (16, 0)
        k = 0
        for x, g in zip(SIXTEEN, got):
            docs = M.accepted(x, columns, M.DELETED)
            assert g.error is None and g.total == len(docs), M.text(x)
            want = M.facets(columns, docs)
            assert {n: v for n, v in g.facets.items() if n in want or n in ("tags", "v32", "big", "none")} == want, M.text(x)
            if x[0] == "scalar":                                           # the scalar facet columns beside them: what they are without any list column
                assert {n: v for n, v in g.facets.items() if n in ("year", "genre")} == scalar[k].facets and g.total == scalar[k].total
                k += 1
        assert k == 2
        sizes = {len(M.accepted(x, columns, M.DELETED)) for x in SIXTEEN}
        assert 0 in sizes and len(live()) in sizes                          # nothing and everything are among them
        again = s.facets_of_documents(exprs)
        assert s.last_filtered_facet_stats()[:2] == (0, 16) and again == got
    finally:
        s.close()


def test_pre_filter_facets_of_a_query(fx):
    e, _, columns = fx
    leaf = L("tags", "=", "t31")
    r = e.search_queries([Query("alpha", 10, pre_filter=M.text(leaf), pre_filter_facets=True)])[0]
    assert r.error is None
    want = M.facets(columns, M.accepted(leaf, columns, M.DELETED))
    assert {n: v for n, v in r.pre_filter_facets.items() if n in ("tags", "v32", "big", "none")} == want
    assert r.pre_filter_facets == e.facets_of_documents(M.text(leaf)).facets
    # the batch's own pre-filter statistics survive the facet call behind it (which takes the masks it needs through the same cache)
    s = Session(e)
    try:
        r = s.search_queries([Query("alpha", 10, pre_filter="year = 2006 AND tags = 't30'", pre_filter_facets=True)])[0]
        assert r.error is None and r.pre_filter_facets is not None and s.last_prefilter_stats() == (1, 0, 1)
    finally:
        s.close()


def test_row_facets_and_browse_facets_leave_list_columns_out(fx):
    e, plain, _ = fx
    qs = [Query("alpha bravo", 64, enable_facets=True), Query("", 64, enable_facets=True), Query("", 64, enable_facets=True, filter="year = 2003")]
    got, want = e.search_queries(qs), plain.search_queries(qs)
    for g, w in zip(got, want):
        assert g.error is None and w.error is None
        assert g.facets == w.facets and set(g.facets) == {"year", "genre"}
        assert_rows(rows_of(g), rows_of(w), "rows")
    browse = e.search_queries([Query("", 64, enable_facets=True, filter="tags = 't31'")])[0]      # the browse FILTER reads the list column; its facets do not
    assert browse.error is None and set(browse.facets) <= {"year", "genre"} and browse.records


def test_two_sessions_return_equal_bytes(fx):
    e, _, _ = fx
    exprs = [M.text(x) for x in SIXTEEN]
    a, b = Session(e), Session(e)
    try:
        assert repr(a.facets_of_all_documents()) == repr(b.facets_of_all_documents())
        one = a.facets_of_documents(exprs)
        e.delete_document_ids([11]); e.restore_documents(); e.delete_document_ids(M.DELETED)      # a new mask epoch: the second session counts again
        two = b.facets_of_documents(exprs)
        assert b.last_filtered_facet_stats()[0] == 16 and repr(one) == repr(two)
    finally:
        a.close(); b.close()
