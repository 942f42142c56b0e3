"""SearchEngine.list_documents on the GPU: a filter's documents in the order of a field, by page.

The expected page is a test-side model: which documents a filter accepts comes from the oracle's filter VM per distinct combination of the values the
expression reads (FilteredModel.accept of tests/test_gpu_filtered_facets.py), the sort keys from tests.bcl_sort (double_key, string_key) or the ints
themselves, dense-ranked; the order is np.lexsort((document, +-rank)) over the accepted live documents and the page its slice.  Every comparison is exact
equality of DocumentKeys, value texts and totals.

70 001 documents (69 tiles of 1024 and a partial one; not a multiple of 4, 16, 64 or 256).  Columns: an int with 100 values, of which one occurs once, at
the last document (its filter accepts the partial last group alone); the int / double / string columns of tests/test_gpu_boost_sort.py (NaN, -0.0 and 0.0;
Drama / drama / DRAMA); a 10-value column whose ties of about 7000 documents lie in every range; a 55 000-value column (two 11-bit digits) and a unique
one (every key distinct, 17 bits: two 11-bit digits, five 4-bit ones; wider keys are walked by tests/test_listing_model.py)."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, ListRequest, Listing
from infidex_amd.engine import Session
from tests import bcl_sort as B
from tests.browse_model import BrowseModel, facet_text
from tests.test_gpu_boost_sort import columns, rows_of
from tests.test_gpu_filtered_facets import FilteredModel
from tools.synth import Synth

pytestmark = pytest.mark.gpu

D = 70001
ONE_PCT, NOTHING, EVERYTHING, LAST_ONLY, TWO_COLS = "shop = 7", "shop < 0", "shop >= 0", "shop = 99", "year >= 2000 AND rating > 7.0"
FILTERS = [None, ONE_PCT, NOTHING, EVERYTHING, LAST_ONLY, TWO_COLS]
ORDERS = ["shop", "year", "rating", "genre", "ten", "wide", "uniq"]


def variant(x, depth=1):
    """The same filter under another cache key."""
    return "(" * depth + x + ")" * depth


def dense_rank(vals):
    if isinstance(vals, np.ndarray) and vals.dtype.kind == "i":
        keys = [int(v) for v in vals]
    elif isinstance(vals, np.ndarray):
        keys = [B.double_key(float(v)) for v in vals]
    else:
        keys = [B.string_key(v) for v in vals]
    rank = {k: i for i, k in enumerate(sorted(set(keys)))}
    return np.asarray([rank[k] for k in keys], np.int64)


class ListModel:
    def __init__(self, cols, keys=None):
        self.fm = FilteredModel(cols, keys)
        self.cols = cols
        self.keys = np.asarray(self.fm.m.keys, np.int64)
        self._rank, self._order = {}, {}

    def set_deleted(self, ids):
        self.fm.set_deleted(ids); self._order = {}

    def add_column(self, name, vals):
        self.fm.add_column(name, vals, False)

    def rank(self, name):
        if name not in self._rank:
            self._rank[name] = dense_rank(self.cols[name][0])
        return self._rank[name]

    def order(self, expr, name, asc):
        """every accepted live document, in the listing's order"""
        k = (expr, name, bool(asc))
        if k not in self._order:
            live = ~self.fm.deleted if expr is None else (self.fm.accept(variantless(expr)) & ~self.fm.deleted)
            d = np.nonzero(live)[0]
            if name is not None:
                r = self.rank(name)[d]
                d = d[np.lexsort((d, r if asc else -r))]
            self._order[k] = d
        return self._order[k]

    def page(self, r):
        d = self.order(r.filter, r.order_by, r.ascending)
        rows = d[r.offset:r.offset + r.limit]
        vals = [] if r.order_by is None else [facet_text(self.cols[r.order_by][0][i]) for i in rows]
        return Listing([int(k) for k in self.keys[rows]], vals, len(d), None)

    def check(self, got, r, ctx=None):
        want = self.page(r)
        assert got.error is None, (ctx, r, got.error)
        assert got.total == want.total, (ctx, r, got.total, want.total)
        assert got.document_ids == want.document_ids, (ctx, r, got.document_ids[:6], want.document_ids[:6], len(got.document_ids), len(want.document_ids))
        assert got.values == want.values, (ctx, r, got.values[:6], want.values[:6])


def variantless(x):
    while x.startswith("(") and x.endswith(")"):
        x = x[1:-1]
    return x


def run(s, m, reqs, ctx=None):
    """lists reqs sixteen at a time on session (or engine) s and holds every page to the model"""
    got = s.list_documents(reqs)
    assert len(got) == len(reqs)
    for g, r in zip(got, reqs):
        m.check(g, r, ctx)
    return got


@pytest.fixture(scope="module")
def fx():
    syn = Synth(2, docs=D)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, syn.field_weights)
    rng = np.random.default_rng(23)
    year, rating, genre = columns(D)
    shop = rng.integers(0, 99, D).astype(np.int64); shop[D - 1] = 99                # 100 values; 99 occurs once, at the last document
    ten = ["c%d" % v for v in rng.integers(0, 10, D)]
    wide = rng.permutation(np.arange(D, dtype=np.int64) % 55000 + 100000)
    uniq = rng.permutation(np.arange(D, dtype=np.int64)) * 3 - 5000
    cols = {"shop": (shop, False), "year": (year, True), "rating": (rating, False), "genre": (genre, True), "ten": (ten, True), "wide": (wide, False), "uniq": (uniq, False)}
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    qa, qo = syn.queries(12, qseed=47, fuzz=0.3)
    return e, ListModel(cols), Synth.texts(qa, qo)


def test_every_column_filter_and_direction(fx):
    e, m, _ = fx
    assert 500 <= m.page(ListRequest(ONE_PCT)).total <= 900 and m.page(ListRequest(LAST_ONLY)).document_ids == [D - 1]
    assert m.page(ListRequest(NOTHING)).total == 0 and m.page(ListRequest(EVERYTHING)).total == D
    s = Session(e)
    try:
        for name in ORDERS:
            reqs = []
            for x in FILTERS:
                for asc in (True, False):
                    total = len(m.order(x, name, asc))
                    reqs += [ListRequest(x, name, asc, 0, 20), ListRequest(x, name, asc, total // 2, 65), ListRequest(x, name, asc, max(total - 1, 0), 64),
                             ListRequest(x, name, asc, total, 20), ListRequest(x, name, asc, max(total - 30, 0), 97)]      # ..., offset = total - 1, >= total, a short last page
            run(s, m, reqs, name)
        # the double column's specials and the string column's case variants are rows like any other
        low = s.list_documents(None, "rating", True, 0, 1024)
        assert low.values[0] == "NaN" and {"NaN", "-0", "0"} <= set(low.values + s.list_documents(None, "rating", True, 1024 * 7, 1024).values)
        g = s.list_documents(None, "genre", True, 0, 1)
        assert g.total == D and g.values == ["Action"]
        seen = []
        for v in m.page(ListRequest(None, "genre", True, 0, D)).values:
            if not seen or seen[-1] != v:
                seen.append(v)
        assert seen[seen.index("Crime") + 1:][:3] == ["DRAMA", "Drama", "drama"]      # OrdinalIgnoreCase-equal, then ordinal
    finally:
        s.close()


def test_limits_and_page_shapes(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        # the 10-value column under accept-everything: ties of about 7000 documents
        o = m.order(EVERYTHING, "ten", True); r = m.rank("ten")[o]
        first_c1 = int(np.searchsorted(r, 1)); last_c1 = int(np.searchsorted(r, 2)) - 1
        assert last_c1 - first_c1 > 6000
        reqs = [ListRequest(EVERYTHING, "ten", True, first_c1 + 1000, lim) for lim in (1, 64, 65, 1024)]          # wholly inside one tie: T_lo == T_hi
        reqs += [ListRequest(EVERYTHING, "ten", True, first_c1, 1024), ListRequest(EVERYTHING, "ten", True, last_c1 - 1023, 1024),   # at the tie's first / last element
                 ListRequest(EVERYTHING, "ten", True, last_c1, 2), ListRequest(EVERYTHING, "ten", True, first_c1 - 1, 2),             # across a key boundary
                 ListRequest(EVERYTHING, "ten", False, D - 1 - last_c1 + 500, 1024), ListRequest(EVERYTHING, "ten", False, 6990, 97)]  # descending: ties still by ascending index
        got = run(s, m, reqs, "ten")
        assert len(set(got[3].values)) == 1 and len(got[3].document_ids) == 1024 and got[3].document_ids == sorted(got[3].document_ids)
        assert got[8].document_ids == sorted(got[8].document_ids) and len(set(got[8].values)) == 1
        # pages spanning several keys (the 100-value column under the two-column filter), limits 1, 64, 65, 1024
        run(s, m, [ListRequest(TWO_COLS, "shop", asc, off, lim) for asc in (True, False) for off in (0, 777) for lim in (1, 64, 65, 1024)], "shop")
        assert len(set(m.page(ListRequest(TWO_COLS, "shop", True, 777, 1024)).values)) > 3
        # the 55 000-value column, two 11-bit digits: first and last key of a page differ in the first digit / only in the last
        o = m.order(EVERYTHING, "wide", True); k = 1 + m.rank("wide")[o]
        cross = int(np.searchsorted(k, 2048 * 9))                                   # the first position whose key has first digit 9
        a, b = ListRequest(EVERYTHING, "wide", True, cross - 5, 64), ListRequest(EVERYTHING, "wide", True, cross + 40, 1024)
        assert k[a.offset] >> 11 != k[a.offset + 63] >> 11 and k[b.offset] >> 11 == k[b.offset + 1023] >> 11 and k[b.offset] != k[b.offset + 1023]
        run(s, m, [a, b, ListRequest(EVERYTHING, "wide", False, cross, 1024), ListRequest(ONE_PCT, "wide", True, 300, 200)], "wide")
        assert s.last_list_stats()[2] == 8                                          # four requests of two passes each
        # every key distinct
        run(s, m, [ListRequest(None, "uniq", True, 33333, 1024), ListRequest(None, "uniq", False, D - 1024, 1024), ListRequest(TWO_COLS, "uniq", False, 5, 65)], "uniq")
        assert s.last_list_stats()[2] == 6                                          # 70 001 values: 17 bits, two digits
    finally:
        s.close()


def test_index_order_equals_browse_from_a_deep_offset(fx):
    e, m, _ = fx
    bm = m.fm.m
    for x in (None, TWO_COLS, ONE_PCT):
        rows = bm.rows(x, D)                                                        # BrowseModel: the live documents the filter accepts, in index order
        off = len(rows) - len(rows) // 3
        got = e.list_documents(x, None, True, off, 1024)
        assert got.error is None and got.values == [] and got.total == len(rows)
        assert got.document_ids == rows[off:off + 1024], x
        assert e.list_documents(x, None, False, off, 50).document_ids == rows[off:off + 50]       # a constant key: descending is index order too
        m.check(got, ListRequest(x, None, True, off, 1024))


def test_consecutive_pages_are_the_whole_order(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        for x, name, asc, upto in ((ONE_PCT, "ten", True, None), (ONE_PCT, "rating", False, None), (EVERYTHING, "ten", True, 3000), (EVERYTHING, "ten", False, 3000)):
            want = [int(k) for k in m.keys[m.order(x, name, asc)]]
            upto = len(want) if upto is None else upto
            reqs = [ListRequest(x, name, asc, off, 97) for off in range(0, upto + 97, 97)]
            got = run(s, m, reqs, (x, name))
            walked = [k for g in got for k in g.document_ids]
            assert walked == want[:len(walked)] and len(walked) >= min(upto, len(want)) and len(set(walked)) == len(walked)
            if upto >= len(want):
                assert walked == want and got[-1].document_ids == []
    finally:
        s.close()


def test_digit_width_changes_the_passes_not_the_pages(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        reqs = [ListRequest(EVERYTHING, "wide", True, 12345, 1024), ListRequest(ONE_PCT, "wide", False, 100, 97), ListRequest(None, "wide", True, D - 3, 64)]
        at11 = run(s, m, reqs, 11)
        assert s.list_documents(ONE_PCT, "shop", True, 0, 20).total and s.last_list_stats()[2] == 1          # 100 values: one pass
        s.list_documents(ONE_PCT, "wide", True, 0, 20)
        assert s.last_list_stats()[2] == 2                                          # 55 000 values: 16 bits, two 11-bit digits
        for bits, passes in ((4, 4), (5, 4)):
            s.set_list_digit_bits(bits)
            assert run(s, m, reqs, bits) == at11
            assert s.last_list_stats()[2] == 3 * passes
            s.list_documents(ONE_PCT, "wide", True, 0, 20)
            assert s.last_list_stats()[2] == passes
            run(s, m, [ListRequest(TWO_COLS, "uniq", False, 4000, 1024), ListRequest(None, "rating", True, 3000, 65), ListRequest(EVERYTHING, "ten", False, 9000, 1024)], bits)
        s.set_list_digit_bits(11)
    finally:
        s.close()


def test_masks_are_reused_and_built_in_one_launch(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        x = variant(ONE_PCT, 2)
        first = s.list_documents(x, "year", True, 0, 20)
        assert s.last_list_stats()[:2] == (1, 0)
        second = s.list_documents(x, "year", True, 20, 20)
        assert s.last_list_stats()[:2] == (0, 1)                                    # the second page of the same filter: nothing built
        m.check(first, ListRequest(x, "year", True, 0, 20)); m.check(second, ListRequest(x, "year", True, 20, 20))
        s.list_documents(None, "year", True, 0, 20)
        assert s.last_list_stats()[:2] == (0, 0)                                    # no filter: the index's Deleted flags, no mask
        sixteen = [ListRequest("shop = %d" % (20 + i), "rating", i % 2 == 0, i, 30 + i) for i in range(16)]
        run(s, m, sixteen, "sixteen")
        assert s.last_list_stats()[:2] == (16, 0) and s.last_prefilter_stats() == (16, 0, 1)       # sixteen distinct filters: one k_filter_mask_multi launch
        run(s, m, sixteen, "sixteen again")
        assert s.last_list_stats()[:2] == (0, 16)
        seventeen = [ListRequest("shop = %d" % (40 + i), "ten", True, 5, 40) for i in range(17)]    # Python splits: 16 + 1
        got = run(s, m, seventeen, "seventeen")
        assert len(got) == 17 and all(g.total for g in got) and s.last_list_stats()[:2] == (1, 0)
    finally:
        s.close()


def test_two_calls_and_two_sessions_return_the_same_pages_and_prefilters_share_the_slots(fx):
    e, m, texts = fx
    reqs = [ListRequest(TWO_COLS, "genre", False, 1000, 1024), ListRequest(ONE_PCT, "uniq", True, 0, 1024), ListRequest(None, "ten", True, 40000, 65),
            ListRequest(EVERYTHING, "wide", False, 54321, 97)]
    s, t = Session(e), Session(e)
    try:
        batch = [Query(texts[i], 10, pre_filter=[ONE_PCT, TWO_COLS, None][i % 3]) for i in range(9)]
        before = s.search_queries(batch)
        a = run(s, m, reqs, "a"); b = s.list_documents(reqs); c = t.list_documents(reqs)
        assert a == b == c
        after = s.search_queries(batch)                                             # the listing took and built masks in the slots the batch uses
        for x, y in zip(before, after):
            assert x.error is None and rows_of(x) == rows_of(y) and x.total_in_pre_filter == y.total_in_pre_filter
        assert before[0].total_in_pre_filter == a[1].total and before[1].total_in_pre_filter == a[0].total
        assert s.list_documents(reqs) == a
    finally:
        s.close(); t.close()


def test_refusals_are_per_request(fx):
    e, m, _ = fx
    reqs = [ListRequest("shop = 31", "year"), ListRequest("shop = ", "year"), ListRequest("ten MATCHES 'c[12]'", "year"), ListRequest("shop = 32", "nosuch"),
            ListRequest("shop = 33", "year", True, 0, 0), ListRequest("shop = 33", "year", True, 0, 1025), ListRequest("nosuch = 3", "year"), ListRequest("shop = 34", "ten", False, 3, 7)]
    got = e.list_documents(reqs)
    assert got[1].error and "syntax" in got[1].error.lower() and got[1].document_ids == [] and got[1].total == 0
    assert got[2].error and "MATCHES" in got[2].error
    assert got[3].error and "nosuch" in got[3].error                                # an unknown order_by field is refused, not "every row null"
    assert got[4].error and got[5].error and "limit" in got[4].error
    for i in (0, 6, 7):
        m.check(got[i], reqs[i])                                                    # an unknown field in the FILTER is null, as the filter VM has it
    assert got[0].total and got[7].total and got[6].total == 0
    assert e.list_documents("shop = ", "year").error == got[1].error


def test_duplicate_keys_every_live_document_is_a_row():
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    keys = [10, 11, 10, 12, 11, 10, 13, 12, 14, 13, 14, 15]
    shade = ["red", "blue", "blue", "red", "red", "green", "blue", "blue", "green", "green", "red", "blue"]
    size = np.asarray([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(k, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i, k in enumerate(keys)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    m = ListModel({"shade": (shade, True), "size": (size, False)}, keys)
    reqs = [ListRequest(x, name, asc, off, 5) for x in (None, "shade = 'red'", "size >= 6") for name in ("shade", "size", None) for asc in (True, False) for off in (0, 3, 11)]
    run(e, m, reqs, "duplicates")
    red = e.list_documents("shade = 'red'", "size", False, 0, 20)
    assert red.document_ids == [14, 11, 12, 10] and red.values == ["11", "5", "4", "1"] and red.total == 4      # documents 10, 4, 3, 0: their OWN shade, one row each
    assert e.list_documents(None, "shade", True, 0, 20).document_ids[:5] == [11, 10, 13, 12, 15]              # blue: documents 1, 2, 6, 7, 11 in index order
    assert e.delete_document_ids([0]) == 1
    m.set_deleted([0])
    run(e, m, reqs, "duplicates, document 0 deleted")
    assert e.list_documents("shade = 'red'", "size", True, 0, 20).document_ids == [12, 11, 14]


def test_deletions_restore_and_a_new_column_invalidate(fx):
    e, m, _ = fx
    s = Session(e)
    try:
        o = m.order(EVERYTHING, "ten", True); r = m.rank("ten")[o]
        first_c1 = int(o[np.searchsorted(r, 1)])                                    # the first document of a tie
        reqs = [ListRequest(EVERYTHING, "ten", True, int(np.searchsorted(r, 1)) - 3, 64), ListRequest(ONE_PCT, "rating", False, 0, 1024), ListRequest(None, "uniq", True, D - 40, 65),
                ListRequest(LAST_ONLY, "shop", True, 0, 5), ListRequest(None, None, True, D - 100, 1024), ListRequest(TWO_COLS, "wide", True, 2000, 97)]
        before = run(s, m, reqs, "live")
        assert s.list_documents(reqs) == before and s.last_list_stats()[:2] == (0, 4)
        gone = sorted(set(range(0, D, 7)) | {D - 1, first_c1})
        try:
            assert e.delete_documents(gone) == len(gone)
            m.set_deleted(gone)
            got = run(s, m, reqs, "deleted")
            assert s.last_list_stats()[:2] == (4, 0)                                # the epoch moved: every mask is built again
            assert got[3].document_ids == [] and got[3].total == 0 and got[2].total == D - len(gone) and first_c1 not in got[0].document_ids
        finally:
            e.restore_documents(); m.set_deleted([])
        assert run(s, m, reqs, "restored") == before
        extra = np.asarray([(d * 7919) % 2500 for d in range(D)], np.int64)        # 2500 values: two digits
        e.set_column("extra", extra, facetable=False); m.cols["extra"] = (extra, False); m.add_column("extra", extra)
        run(s, m, [ListRequest(ONE_PCT, "extra", True, 10, 200), ListRequest("extra < 100 AND shop < 50", "extra", False, 0, 1024), ListRequest(None, "extra", True, 50000, 64)] + reqs, "new column")
        assert s.last_list_stats()[:2] == (5, 0)
    finally:
        s.close()
