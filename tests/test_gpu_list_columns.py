"""List columns in filters on the GPU (SearchEngine.set_list_column): every leaf over a list column holds for a document when it holds for at least one
element — for an empty list, when it holds for a null value.

The model is tests/list_column_model.py: a plain Python walk over constructed lists, 1 031 documents (no multiple of 4, 64 or 256) with empty lists at
both ends and in a run of 70, lists of 1, 63, 64, 65 and 300 elements, a list of one repeated value, an empty-string element, a column that is empty for
every document, and dictionaries of 1, 31, 32, 33 values and one above k_list_leaf's LDS bitmap budget (read from include/infidex_hip.h), so that the
bitmaps are read from global memory there.  A few documents are deleted.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import Session, InfidexError
from tests import list_column_model as M
from tests.test_gpu_boost_sort import rows_of, assert_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ECAPACITY = 4
LDS_WORDS = int(re.search(r"#define INFX_LIST_LEAF_LDS_WORDS (\d+)", open(os.path.join(ROOT, "include", "infidex_hip.h")).read()).group(1))
BIG = 32 * LDS_WORDS + 1                   # one leaf's bitmap no longer fits the budget

L = lambda col, op, *args: ("leaf", col, op, args)
YEAR = ("scalar", "year", "=", 2003)
LEAVES = [
    L("v32", "=", 5), L("v32", "!=", 5), L("v32", "<", 3), L("v32", ">=", 30), L("v32", "BETWEEN", 10, 12), L("v32", "IN", 1, 2, 31),
    L("v31", "=", 30), L("v31", "<", 1), L("one", "=", 0), L("one", ">=", 1), L("big", "=", BIG - 1), L("big", "<", 64), L("big", "IN", 0, 4097, BIG - 2),
    L("tags", "=", "t31"), L("tags", "IN", "t30", "t31"), L("tags", "CONTAINS", "3"), L("tags", "STARTS WITH", "t1"), L("tags", "IS NULL"), L("tags", "=", ""),
    L("none", "IS NULL"), L("none", "=", "x"), L("none", "<", "x"),
]


def documents():
    return [Document(d, "alpha bravo item %d" % d) for d in range(M.N)]


def make_engine(columns):
    e = SearchEngine.create_default(device=0)
    e.index_documents(documents())
    e.set_column("year", np.asarray([M.year_of(d) for d in range(M.N)], np.int64), facetable=True)
    for name, (lists, facetable) in columns.items():
        e.set_list_column(name, lists, facetable=facetable)
    return e


@pytest.fixture(scope="module")
def fx():
    columns = M.corpus(BIG)
    e = make_engine(columns)
    # the model's verdicts of two leaves as scalar columns: what the list-column filter must be indistinguishable from
    for name, leaf in (("m_t31", L("tags", "=", "t31")), ("m_t05", L("tags", "=", "t05"))):
        e.set_column(name, np.asarray([int(M.holds(leaf, columns, d)) for d in range(M.N)], np.int64))
    assert e.delete_document_ids(M.DELETED) == len(M.DELETED)
    e.set_filter_cache_limit(4)            # compiled filters leave the cache early, and with them their hold on the 16 derived columns
    yield e, columns
    e.close()


def expected_mask(x, columns):
    live = set(M.accepted(x, columns, M.DELETED))
    return np.asarray([0 if d in live else 1 for d in range(M.N)], np.uint8)


def test_the_corpus_is_what_the_kernels_need(fx):
    _, columns = fx
    tags = columns["tags"][0]
    assert tags[0] == [] and tags[-1] == [] and all(tags[d] == [] for d in M.EMPTY_RUN) and len(M.EMPTY_RUN) == 70
    assert {len(tags[d]) for d in (1, 2, 3, 4, 6)} == {1, 63, 64, 65, 300}
    assert len(set(tags[M.DUPLICATES])) == 1 and len(tags[M.DUPLICATES]) > 1 and "" in tags[8]
    sizes = {name: len({x for l in lists for x in l}) for name, (lists, _) in columns.items()}
    assert sizes == {"tags": 33, "one": 1, "v31": 31, "v32": 32, "big": BIG, "none": 0}


@pytest.mark.parametrize("leaf", LEAVES, ids=M.text)
def test_masks_equal_the_model(fx, leaf):
    """Each leaf alone, under NOT, and under AND / OR with a scalar-column leaf, on every document."""
    e, columns = fx
    s = Session(e)
    try:
        for x in (leaf, ("not", leaf), ("and", leaf, YEAR), ("or", YEAR, leaf), ("and", ("not", leaf), ("not", YEAR))):
            want = expected_mask(x, columns)
            got = s.prefilter_mask(M.text(x))
            assert np.array_equal(got, want), (M.text(x), np.flatnonzero(got != want)[:10])
    finally:
        s.close()


def test_not_equal_means_no_element_equals(fx):
    """`tags != 't05'` is NOT over an = leaf: it accepts the documents none of whose elements is t05 — the empty lists among them — and so does
    NOT tags = 't05'; a document with t05 and another tag is in neither."""
    e, columns = fx
    ne, no = e.prefilter_mask("tags != 't05'"), e.prefilter_mask("NOT tags = 't05'")
    assert np.array_equal(ne, no) and np.array_equal(ne, expected_mask(L("tags", "!=", "t05"), columns))
    tags = columns["tags"][0]
    both = [d for d in range(M.N) if "t05" in tags[d] and len(set(tags[d])) > 1 and d not in M.DELETED]
    assert both and all(ne[d] == 1 for d in both) and ne[1] == 0 and ne[M.EMPTY_RUN[0]] == 0


def test_pre_filter_counts_and_listing_follow_the_model(fx):
    e, columns = fx
    for leaf in (L("tags", "=", "t31"), L("v32", "BETWEEN", 10, 12), L("tags", "IS NULL"), L("big", "<", 64)):
        want = M.accepted(leaf, columns, M.DELETED)
        r = e.search_queries([Query("alpha", 10, pre_filter=M.text(leaf))])[0]
        assert r.error is None and r.total_in_pre_filter == len(want), (M.text(leaf), r.total_in_pre_filter, len(want))
        assert all(x.document_id in set(want) for x in r.records)
        got, off = [], 0
        while True:
            page = e.list_documents(filter=M.text(leaf), offset=off, limit=1024)
            assert page.error is None and page.total == len(want)
            got += page.document_ids; off += 1024
            if off >= page.total:
                break
        assert got == want, M.text(leaf)


def test_post_filter_keeps_exactly_the_models_rows_in_their_order(fx):
    e, columns = fx
    leaf = L("tags", "=", "t31")
    live = set(M.accepted(leaf, columns, M.DELETED))
    plain, filtered, scalar = e.search_queries([Query("alpha bravo", 64), Query("alpha bravo", 64, filter=M.text(leaf)), Query("alpha bravo", 64, filter="m_t31 = 1")])
    assert plain.error is None and filtered.error is None and len(plain.records) == 64
    want = [r for r in rows_of(plain) if r[0] in live]
    assert 0 < len(want) < 64
    assert_rows(rows_of(filtered), want, "post-filter")
    assert_rows(rows_of(filtered), rows_of(scalar), "list leaf against the model's scalar column")
    assert filtered.total_in_filter == scalar.total_in_filter == len(live)


def test_a_boost_raises_exactly_the_models_rows(fx):
    e, columns = fx
    leaf = L("tags", "=", "t05")
    hit = set(M.accepted(leaf, columns, M.DELETED))
    q = lambda f: Query("alpha bravo", 64, enable_boost=True, boosts=[Boost(f, BoostStrength.High)] if f else None)
    plain, boosted, scalar = e.search_queries([q(None), q(M.text(leaf)), q("m_t05 = 1")])
    assert boosted.error is None and {k for k, _, _ in rows_of(plain)} == {k for k, _, _ in rows_of(boosted)}
    before = {k: s for k, s, _ in rows_of(plain)}
    raised = {k for k, s, _ in rows_of(boosted) if s != before[k]}
    assert raised == {k for k in before if k in hit} and raised
    assert all(s > before[k] for k, s, _ in rows_of(boosted) if k in raised)
    assert_rows(rows_of(boosted), rows_of(scalar), "list leaf against the model's scalar column")


@pytest.fixture(scope="module")
def cache_fx():
    """An engine of its own for the tests that count derived columns: nothing else holds one."""
    columns = M.corpus(33)
    columns = {name: (columns[name][0], False) for name in ("tags", "v31", "v32")}
    e = make_engine(columns)
    assert e.delete_document_ids(M.DELETED) == len(M.DELETED)
    yield e, columns
    e.close()


def flush_filters(e, limit):
    """Empties the engine's filter cache of everything that holds a derived column (the cached derived columns themselves stay), then sets its limit."""
    e.set_filter_cache_limit(1)
    e.prefilter_mask("year >= 0")
    e.set_filter_cache_limit(limit)


def test_sixteen_leaves_take_one_launch_and_a_repeat_takes_none(cache_fx):
    e, columns = cache_fx
    leaves = [L("v32", "=", 16 + i) for i in range(16)]
    tree = leaves[0]
    for l in leaves[1:]:
        tree = ("or", tree, l)
    x = M.text(tree)
    flush_filters(e, 64)
    s = Session(e); s2 = Session(e)
    try:
        got = s.prefilter_mask(x)
        assert e.last_list_leaf_stats() == (16, 1)
        assert np.array_equal(got, expected_mask(tree, columns))
        totals = e.list_leaf_totals()
        assert np.array_equal(s2.prefilter_mask(x), got)                # a mask built again, from the cached program
        assert s2.last_prefilter_stats()[0] == 1 and e.list_leaf_totals() == totals      # nothing built, nothing launched
        assert e.last_list_leaf_stats() == (16, 1)                      # (still the last expression that was compiled)
        # leaves over two more list columns: one launch per column, and only for what is missing; three unused columns make room
        flush_filters(e, 64)
        y = ("and", ("and", leaves[0], L("tags", "=", "t07")), ("and", L("v31", "=", 3), L("v31", "=", 4)))
        assert np.array_equal(s.prefilter_mask(M.text(y)), expected_mask(y, columns))
        assert e.last_list_leaf_stats() == (3, 2) and e.list_leaf_totals() == (totals[0] + 3, totals[1] + 2)
    finally:
        s.close(); s2.close()


def test_cache_eviction_and_refusal_when_nothing_is_free(cache_fx):
    """Sixteen derived columns held by cached filters: an expression with a seventeenth leaf is refused alone (INFX_ECAPACITY), its neighbours in the call
    are answered.  Once cached filters have left, the seventeenth evicts the least recently used unused column; the evicted leaf is built again on its
    next use.  An expression with seventeen distinct leaves of its own is always refused."""
    e, columns = cache_fx
    flush_filters(e, 64)
    singles = [L("v31", "=", i) for i in range(16)]
    got = e.facets_of_documents([M.text(l) for l in singles])
    assert [g.error for g in got] == [None] * 16
    for l, g in zip(singles, got):
        assert g.total == len(M.accepted(l, columns, M.DELETED))
    extra = L("v31", "=", 16)
    year = "year = 2001"
    got = e.facets_of_documents([M.text(singles[3]), M.text(extra), year, "(%s) OR %s" % (M.text(extra), year)])
    assert got[0].error is None and got[2].error is None and got[0].total == len(M.accepted(singles[3], columns, M.DELETED))
    assert got[2].total == sum(1 for d in range(M.N) if M.year_of(d) == 2001 and d not in M.DELETED)
    assert got[1].error is not None and "derived" in got[1].error and got[3].error is not None
    with pytest.raises(InfidexError) as ei:
        e.prefilter_mask(M.text(extra))
    assert ei.value.code == ECAPACITY
    # the cached filters leave: the seventeenth takes the least recently used column, the others are still there
    flush_filters(e, 64)
    assert np.array_equal(e.prefilter_mask(M.text(extra)), expected_mask(extra, columns)) and e.last_list_leaf_stats() == (1, 1)
    y2001 = ("scalar", "year", "=", 2001)
    last = ("and", singles[15], y2001)
    assert np.array_equal(e.prefilter_mask(M.text(last)), expected_mask(last, columns))
    assert e.last_list_leaf_stats() == (0, 0)                           # still cached
    first = ("and", singles[0], y2001)                                  # the evicted one
    assert np.array_equal(e.prefilter_mask(M.text(first)), expected_mask(first, columns))
    assert e.last_list_leaf_stats() == (1, 1)
    flush_filters(e, 64)
    with pytest.raises(InfidexError) as ei:
        e.prefilter_mask(" OR ".join(M.text(L("v32", "=", i)) for i in range(17)))
    assert ei.value.code == ECAPACITY
    assert np.array_equal(e.prefilter_mask(M.text(first)), expected_mask(first, columns))      # and the engine goes on
    # a filter cache smaller than a call: the call's expressions stay pinned until the device has counted, so the new leaf of a later expression cannot
    # take a derived column from an earlier one of the same call — it is refused alone, and the earlier answer is the model's
    flush_filters(e, 1)
    wide = L("v32", "=", 16)
    for i in range(17, 32):
        wide = ("or", wide, L("v32", "=", i))
    got = e.facets_of_documents([M.text(wide), "year = 2002", M.text(L("v32", "=", 3))])
    assert got[0].error is None and got[0].total == len(M.accepted(wide, columns, M.DELETED))
    assert got[1].error is None and got[2].error is not None and "derived" in got[2].error
    e.set_filter_cache_limit(64)
    assert e.facets_of_documents(M.text(L("v32", "=", 3))).total == len(M.accepted(L("v32", "=", 3), columns, M.DELETED))      # once the call is over there is room


def test_mostly_cached_leaves_are_not_rebuilt_for_a_missing_one(cache_fx):
    """Sixteen cached, unused derived columns; an expression that reads fifteen of them and one new leaf, the new leaf FIRST: the fifteen are kept while
    room is made, so exactly one column is built."""
    e, columns = cache_fx
    flush_filters(e, 64)
    sixteen = [L("v31", "=", i) for i in range(16)]
    for l in sixteen:
        e.prefilter_mask(M.text(l))
    flush_filters(e, 64)
    tree = L("v31", "=", 20)
    for l in sixteen[1:]:
        tree = ("or", tree, l)
    totals = e.list_leaf_totals()
    assert np.array_equal(e.prefilter_mask(M.text(tree)), expected_mask(tree, columns))
    assert e.last_list_leaf_stats() == (1, 1) and e.list_leaf_totals() == (totals[0] + 1, totals[1] + 1)


def test_one_session_lowers_new_leaves_while_another_filters_browses_and_counts(fx):
    """Two threads, a session each: one keeps compiling expressions with list-column leaves the engine has not seen (every one a k_list_leaf launch into a
    new or reused slot of the column table), the other runs a pre-filtered query, a browse query and a filtered-facet call over and over.  Nothing is
    refused, and every answer is what it is without the other thread."""
    import threading
    e, columns = fx
    a, b = Session(e), Session(e)
    pre = Query("alpha bravo", 10, pre_filter="year = 2003")
    browse = Query("", 20, enable_facets=True, filter="year >= 2004")
    base = b.search_queries([pre, browse])
    assert all(r.error is None for r in base)
    want_total = b.facets_of_documents("year = 2005").total
    errors, rounds, stop = [], [0], threading.Event()

    def lower():
        try:
            for i in range(180):                                         # 180 distinct leaves: the sixteen slots are rewritten eleven times over
                leaf = L("v32" if i % 2 else "v31", ("=", "<", ">=")[i % 3], i // 6)
                x = ("and", leaf, ("scalar", "year", ">=", 2000 + i % 5))
                got = a.prefilter_mask(M.text(x))
                if not np.array_equal(got, expected_mask(x, columns)):
                    errors.append(("mask", M.text(x)))
        except Exception as ex:                                          # noqa: BLE001 (whatever it is, the test reports it)
            errors.append(("lower", repr(ex)))
        finally:
            stop.set()

    def serve():
        try:
            while not stop.is_set() or rounds[0] < 3:
                got = b.search_queries([pre, browse])
                for g, w in zip(got, base):
                    if g.error is not None or rows_of(g) != rows_of(w) or g.facets != w.facets or g.total_in_pre_filter != w.total_in_pre_filter:
                        errors.append(("search", g.error))
                f = b.facets_of_documents("(" * (rounds[0] % 40 + 1) + "year = 2005" + ")" * (rounds[0] % 40 + 1))
                if f.error is not None or f.total != want_total:
                    errors.append(("facets", f.error, f.total))
                rounds[0] += 1
        except Exception as ex:                                          # noqa: BLE001
            errors.append(("serve", repr(ex)))

    t1, t2 = threading.Thread(target=lower), threading.Thread(target=serve)
    t1.start(); t2.start(); t1.join(120); t2.join(120)
    a.close(); b.close()
    assert not t1.is_alive() and not t2.is_alive()
    assert not errors, errors[:5]
    assert rounds[0] >= 3


def test_a_list_column_is_an_unknown_field_to_orders_groups_and_aggregates(fx):
    e, _ = fx
    for got in (e.list_documents(order_by="tags"), e.list_groups(group_by="tags"), e.field_stats(field="v32"), e.top_groups(group_by="tags")):
        assert got.error is not None and "named" in got.error, got.error
    assert e.list_documents(order_by="year").error is None
    assert e.bucket_stats(field="year", bucket_by="v32", edges=(1.0, 2.0)).error is not None
    assert e.bucket_stats(field="v32", bucket_by="year", edges=(2001.0, 2003.0)).error is not None
    r = e.search_queries([Query("alpha", 10, sort_by="tags"), Query("alpha", 10, collapse_by="tags"), Query("alpha", 10, sort_by="year"), Query("alpha", 10, sort_by="nosuch")])
    assert r[0].error is not None and "list column" in r[0].error and r[1].error is not None and "named" in r[1].error
    assert r[2].error is None and r[3].error is None and r[2].records and r[3].records      # a scalar field, and a field nobody has, sort as before


def test_replacing_the_list_column_changes_the_answers():
    columns = M.corpus(33)
    e = make_engine({"tags": columns["tags"]})
    try:
        leaf = L("tags", "=", "t31")
        assert np.array_equal(e.prefilter_mask(M.text(leaf)), np.asarray([0 if M.holds(leaf, columns, d) else 1 for d in range(M.N)], np.uint8))
        assert e.facets_of_documents(M.text(leaf)).total == len(M.accepted(leaf, columns))
        flipped = {"tags": ([list(reversed(columns["tags"][0][M.N - 1 - d])) for d in range(M.N)], True)}
        e.set_list_column("tags", flipped["tags"][0], facetable=True)
        assert e.list_column("tags", M.N - 1 - 8) == ["t02", ""]
        want = np.asarray([0 if M.holds(leaf, flipped, d) else 1 for d in range(M.N)], np.uint8)
        got = e.prefilter_mask(M.text(leaf))
        assert np.array_equal(got, want) and not np.array_equal(got, got[::-1])
        assert e.last_list_leaf_stats() == (1, 1)                       # the derived column went with the old lists
        assert e.facets_of_documents(M.text(leaf)).facets["tags"] == M.facets(flipped, M.accepted(leaf, flipped))["tags"]
        # ... and a scalar column of the same name replaces the list column: the leaf reads one value per document again
        e.set_column("tags", ["t31" if d % 2 else "x" for d in range(M.N)])
        assert np.array_equal(e.prefilter_mask(M.text(leaf)), np.asarray([0 if d % 2 else 1 for d in range(M.N)], np.uint8))
        assert e.last_list_leaf_stats() == (0, 0)
    finally:
        e.close()
