"""SearchEngine.list_groups on the GPU: one row per value of a field — the group's first document in the order of a field — by page, with the groups' sizes.

The expected page is a test-side model on top of tests/test_gpu_list_documents.py's ListModel: ListModel.order(filter, order_by, ascending) is every accepted
live document in the listing's order; the heads are the first occurrence of each group along that order, the page their slice, the sizes a count per group.
Every comparison is exact equality of DocumentKeys, value texts, group texts, sizes and totals.  Group identity is pinned to field_stats, not to the model's
own idea of equality: for the group columns field_stats takes (at most 4096 values — `mid`, `wide` and `uniq` are beyond it and rest on the model alone),
{group_values: group_sizes} over all pages equals {g.value: g.count + g.nan} of field_stats(filter, "shop", group_by) and total_groups its number of groups.

The corpus and the columns are test_gpu_list_documents.py's (70 001 documents: 69 full tiles and a partial one, no multiple of 4 or 16), with a constant
column and `mid` (12 000 values).  The head table of a group column lies in a workgroup's LDS up to 8 191 values (ten, shop, genre, rating, one), in the
whole LDS of a CU up to 20 479 (mid), in global memory beyond (wide: 55 000, uniq: 70 001)."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, GroupListRequest, GroupListing, ListRequest
from infidex_amd.engine import Session
from tests.browse_model import facet_text
from tests.test_gpu_boost_sort import columns
from tests.test_gpu_list_documents import ListModel, D, ONE_PCT, NOTHING, EVERYTHING, LAST_ONLY, TWO_COLS, FILTERS, variant
from tools.synth import Synth

pytestmark = pytest.mark.gpu

GROUPS = ["ten", "shop", "genre", "rating", "mid", "wide", "uniq", "one"]
ORDERS = [None, "ten", "rating", "genre", "wide", "uniq"]
STATS_GROUPS = ["ten", "shop", "genre", "rating", "one"]      # field_stats groups by at most 4096 values


class GroupModel:
    def __init__(self, lm):
        self.lm = lm
        self._gid, self._heads = {}, {}

    def set_deleted(self, ids):
        self.lm.set_deleted(ids); self._heads = {}

    def set_column(self, name, vals):
        self.lm.cols[name] = (vals, False); self._gid.pop(name, None); self._heads = {}

    def gid(self, g):
        """per document the number of its group, and the groups' texts: a group is one facet text of the column"""
        if g not in self._gid:
            names, ids = {}, np.zeros(len(self.lm.cols[g][0]), np.int64)
            for d, v in enumerate(self.lm.cols[g][0]):
                ids[d] = names.setdefault(facet_text(v), len(names))
            self._gid[g] = (ids, list(names))
        return self._gid[g]

    def heads(self, x, g, c, asc):
        """(the heads in the listing's order, every group's size by group number, the size of the set)"""
        k = (x, g, c, bool(asc))
        if k not in self._heads:
            o = self.lm.order(x, c, asc)
            ids, names = self.gid(g)
            _, first = np.unique(ids[o], return_index=True)
            self._heads[k] = (o[np.sort(first)], np.bincount(ids[o], minlength=len(names)), len(o))
        return self._heads[k]

    def page(self, r):
        h, sizes, total = self.heads(r.filter, r.group_by, r.order_by, r.ascending)
        ids, names = self.gid(r.group_by)
        rows = h[r.offset:r.offset + r.limit]
        vals = [] if r.order_by is None else [facet_text(self.lm.cols[r.order_by][0][i]) for i in rows]
        return GroupListing([int(k) for k in self.lm.keys[rows]], vals, [names[ids[i]] for i in rows], [int(sizes[ids[i]]) for i in rows], len(h), total, None)

    def check(self, got, r, ctx=None):
        want = self.page(r)
        assert got.error is None, (ctx, r, got.error)
        assert (got.total_groups, got.total) == (want.total_groups, want.total), (ctx, r, got.total_groups, got.total, want.total_groups, want.total)
        assert got.document_ids == want.document_ids, (ctx, r, got.document_ids[:6], want.document_ids[:6], len(got.document_ids), len(want.document_ids))
        assert got.values == want.values, (ctx, r, got.values[:6], want.values[:6])
        assert got.group_values == want.group_values, (ctx, r, got.group_values[:6], want.group_values[:6])
        assert got.group_sizes == want.group_sizes, (ctx, r, got.group_sizes[:6], want.group_sizes[:6])


def run(s, gm, reqs, ctx=None):
    """lists reqs sixteen at a time on session (or engine) s and holds every page to the model"""
    got = s.list_groups(reqs)
    assert len(got) == len(reqs)
    for g, r in zip(got, reqs):
        gm.check(g, r, ctx)
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
    mid = rng.permutation(np.arange(D, dtype=np.int64) % 12000) * 7 + 1
    one = np.full(D, 42, np.int64)
    cols = {"shop": (shop, False), "year": (year, True), "rating": (rating, False), "genre": (genre, True), "ten": (ten, True), "wide": (wide, False), "uniq": (uniq, False),
            "mid": (mid, False), "one": (one, False)}
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    lm = ListModel(cols)
    return e, lm, GroupModel(lm)


def test_the_group_columns_reach_every_placement(fx):
    _, _, gm = fx
    card = {g: len(gm.gid(g)[1]) for g in GROUPS}
    assert card["ten"] == 10 and card["shop"] == 100 and card["one"] == 1 and card["mid"] == 12000 and card["wide"] == 55000 and card["uniq"] == D
    assert {"Drama", "drama", "DRAMA"} <= set(gm.gid("genre")[1]) and {"NaN", "-0", "0"} <= set(gm.gid("rating")[1])
    assert all(card[g] <= 8191 for g in STATS_GROUPS) and 8191 < card["mid"] <= 20479 < card["wide"]


@pytest.mark.parametrize("g", GROUPS)
def test_every_filter_order_and_direction(fx, g):
    e, lm, gm = fx
    s = Session(e)
    try:
        for c in ORDERS:
            reqs = []
            for x in FILTERS:
                for asc in (True, False):
                    tg = len(gm.heads(x, g, c, asc)[0])
                    reqs += [GroupListRequest(x, g, c, asc, 0, 20), GroupListRequest(x, g, c, asc, tg // 2, 65), GroupListRequest(x, g, c, asc, max(tg - 30, 0), 97),
                             GroupListRequest(x, g, c, asc, tg, 20)]      # ..., a short last page, offset == total_groups
            got = run(s, gm, reqs, (g, c))
            assert s.last_group_list_stats()[2] == 4                      # the last sixteen requests: four pages of each of four listings
            for k, x in enumerate(FILTERS):
                first = got[8 * k]
                if x == NOTHING:
                    assert first.total_groups == first.total == 0 and first.document_ids == [] and first.error is None
                if x == LAST_ONLY:
                    assert first.document_ids == [D - 1] and first.group_sizes == [1] and first.total_groups == first.total == 1
    finally:
        s.close()


@pytest.mark.parametrize("g", STATS_GROUPS)
def test_groups_are_field_stats_groups(fx, g):
    e, lm, gm = fx
    for x in FILTERS:
        st = e.field_stats(x, "shop", g)
        assert st.error is None
        want = {grp.value: grp.count + grp.nan for grp in st.groups}
        assert len(want) == len(st.groups)                                # (no two groups share a text)
        for c, asc in ((None, True), ("rating", False)):
            got = e.list_groups(x, g, c, asc, 0, 1024)
            assert got.error is None and got.total_groups == len(st.groups) == len(got.document_ids) and got.total == st.total
            assert dict(zip(got.group_values, got.group_sizes)) == want, (x, g, c)


def test_heads_under_ties_are_the_lowest_index(fx):
    e, lm, gm = fx
    shop, ten_rank = lm.cols["shop"][0], lm.rank("ten")
    live = np.arange(D)                                                      # EVERYTHING: some 700 members per shop, ties of about 70 at every key
    for asc in (True, False):
        want = {}
        for v in np.unique(shop[live]):
            mem = live[shop[live] == v]
            best = ten_rank[mem].min() if asc else ten_rank[mem].max()
            tied = mem[ten_rank[mem] == best]
            assert len(tied) > 20 or len(mem) == 1                       # the best key is shared (shop 99 has one member)
            want[str(int(v))] = int(tied.min())                          # ties go by ascending index in both directions (keys are indices here)
        got = e.list_groups(EVERYTHING, "shop", "ten", asc, 0, 1024)
        assert dict(zip(got.group_values, got.document_ids)) == want and got.total_groups == len(want) == 100
        assert got.values == sorted(got.values, reverse=not asc)
        gm.check(got, GroupListRequest(EVERYTHING, "shop", "ten", asc, 0, 1024))
    # without order_by: the first member in index order, the rows in index order
    live = np.nonzero(lm.fm.accept(TWO_COLS))[0]
    got = e.list_groups(TWO_COLS, "shop", None, True, 0, 1024)
    assert dict(zip(got.group_values, got.document_ids)) == {str(int(v)): int(live[shop[live] == v].min()) for v in np.unique(shop[live])}
    assert got.document_ids == sorted(got.document_ids) and got.values == [] and len(got.document_ids) > 90
    assert e.list_groups(TWO_COLS, "shop", None, False, 0, 1024) == got


def test_group_by_a_unique_column_is_list_documents(fx):
    e, lm, gm = fx
    pages = [(None, "uniq", True, 33333, 1024), (TWO_COLS, "rating", False, 1000, 97), (ONE_PCT, None, True, 0, 1024), (EVERYTHING, "ten", False, 6990, 65),
             (LAST_ONLY, "genre", True, 0, 20), (NOTHING, "wide", True, 0, 20), (None, "wide", False, D - 5, 64)]
    got = e.list_groups([GroupListRequest(x, "uniq", c, asc, off, lim) for x, c, asc, off, lim in pages])
    want = e.list_documents([ListRequest(x, c, asc, off, lim) for x, c, asc, off, lim in pages])
    for g, w, p in zip(got, want, pages):
        assert g.error is None and w.error is None
        assert (g.document_ids, g.values, g.total) == (w.document_ids, w.values, w.total), p
        assert g.total_groups == g.total and g.group_sizes == [1] * len(g.document_ids), p
        lm.check(w, ListRequest(*p))


def test_a_constant_column_is_one_row_the_first_of_list_documents(fx):
    e, lm, gm = fx
    for x in (None, ONE_PCT, EVERYTHING, LAST_ONLY, TWO_COLS):
        for c, asc in ((None, True), ("rating", True), ("uniq", False), ("ten", False)):
            g = e.list_groups(x, "one", c, asc, 0, 20)
            w = e.list_documents(x, c, asc, 0, 1)
            assert g.error is None and g.total_groups == 1 and g.total == w.total and g.group_sizes == [w.total] and g.group_values == ["42"]
            assert (g.document_ids, g.values) == (w.document_ids, w.values), (x, c, asc)
    g = e.list_groups(NOTHING, "one", "rating", True, 0, 20)
    assert g.error is None and g.total_groups == g.total == 0 and g.document_ids == g.values == g.group_values == g.group_sizes == []


def test_offsets_at_and_beyond_the_groups_are_empty_pages(fx):
    e, lm, gm = fx
    tg = len(gm.heads(TWO_COLS, "shop", "rating", True)[0])
    reqs = [GroupListRequest(TWO_COLS, "shop", "rating", True, off, 20) for off in (tg - 1, tg, tg + 1, D, 2 ** 31 - 1)]
    got = run(e, gm, reqs, "offsets")
    assert len(got[0].document_ids) == 1 and all(g.document_ids == [] and g.total_groups == tg and g.total == got[0].total and g.error is None for g in got[1:])


def test_consecutive_pages_are_the_whole_head_order_and_the_sizes_add_up(fx):
    e, lm, gm = fx
    s = Session(e)
    try:
        for x, g, c, asc, lim in ((EVERYTHING, "ten", "uniq", False, 1), (TWO_COLS, "shop", "rating", True, 1), (None, "mid", "wide", True, 1024), (ONE_PCT, "wide", "genre", False, 97),
                                  (TWO_COLS, "mid", None, True, 97), (None, "rating", "ten", False, 97)):
            h, sizes, total = gm.heads(x, g, c, asc)
            reqs = [GroupListRequest(x, g, c, asc, off, lim) for off in range(0, len(h) + lim, lim)]
            got = run(s, gm, reqs, (x, g, c))
            walked = [k for p in got for k in p.document_ids]
            assert walked == [int(k) for k in lm.keys[h]] and len(set(walked)) == len(walked) and got[-1].document_ids == []
            assert sum(n for p in got for n in p.group_sizes) == total == got[0].total
            assert len({v for p in got for v in p.group_values}) == len(h) == got[0].total_groups
    finally:
        s.close()


def test_the_same_bytes_alone_among_sixteen_on_two_sessions_and_at_any_digit_width(fx):
    e, lm, gm = fx
    s, t = Session(e), Session(e)
    try:
        probe = GroupListRequest(TWO_COLS, "mid", "wide", False, 2000, 1024)
        alone = s.list_groups([probe])[0]
        gm.check(alone, probe)
        others = [GroupListRequest([ONE_PCT, None, EVERYTHING][i % 3], GROUPS[i % 8], ORDERS[i % 6], i % 2 == 0, 3 * i, 40 + i) for i in range(15)]
        for at in (0, 7, 15):
            among = run(s, gm, others[:at] + [probe] + others[at:], at)
            assert repr(among[at]) == repr(alone)
        assert repr(t.list_groups([probe])[0]) == repr(alone)
        for bits in (4, 11):
            s.set_list_digit_bits(bits)
            assert repr(s.list_groups([probe])[0]) == repr(alone), bits
            assert repr(run(s, gm, others, bits)) == repr(t.list_groups(others))
    finally:
        s.close(); t.close()


def test_head_passes_and_masks_are_shared(fx):
    e, lm, gm = fx
    s = Session(e)
    try:
        x = variant(ONE_PCT, 3)
        pages = [GroupListRequest(x, "mid", "rating", True, 40 * i, 40) for i in range(16)]
        run(s, gm, pages, "sixteen pages")
        built, reused, heads, hist, launches = s.last_group_list_stats()
        assert (built, reused, heads) == (1, 0, 1) and hist == 16                  # ONE head pass for sixteen pages of one listing; rating: one digit each
        assert launches == 1 + 2 + 16 * 6 + 2                                      # mask build; heads, heads mask; per page hist, pick, count, prefix, gather, sort; page codes, sizes
        run(s, gm, pages[:3] + [GroupListRequest(x, "mid", "rating", False, 0, 40), GroupListRequest(x, "shop", "rating", True, 0, 40)], "three listings")
        assert s.last_group_list_stats()[:3] == (0, 1, 3)                          # the other direction and another group column are listings of their own
        sixteen = [GroupListRequest("shop = %d" % (20 + i), "ten", "rating", i % 2 == 0, i % 3, 5 + i) for i in range(16)]
        run(s, gm, sixteen, "sixteen filters")
        assert s.last_group_list_stats()[:3] == (16, 0, 16) and s.last_prefilter_stats() == (16, 0, 1)      # sixteen distinct filters: one k_filter_mask_multi launch
        run(s, gm, sixteen, "sixteen filters again")
        assert s.last_group_list_stats()[:3] == (0, 16, 16)
        run(s, gm, [GroupListRequest(None, "ten", None, True, 0, 5)], "no filter")
        assert s.last_group_list_stats()[:3] == (0, 0, 1)                          # the index's Deleted flags, no mask
        seventeen = [GroupListRequest("shop = %d" % (40 + i), "genre", "ten", True, 1, 40) for i in range(17)]      # Python splits: 16 + 1
        got = run(s, gm, seventeen, "seventeen")
        assert len(got) == 17 and all(p.total_groups for p in got) and s.last_group_list_stats()[:3] == (1, 0, 1)
        # the mask list_documents built serves list_groups
        y = variant(TWO_COLS, 2)
        assert s.list_documents(y, "year", True, 0, 20).total == s.list_groups(y, "shop", "year", True, 0, 20).total
        assert s.last_group_list_stats()[:2] == (0, 1)
    finally:
        s.close()


def test_refusals_are_per_request(fx):
    e, lm, gm = fx
    reqs = [GroupListRequest("shop = 31", "ten", "year"), GroupListRequest("shop = ", "ten", "year"), GroupListRequest("ten MATCHES 'c[12]'", "ten", "year"),
            GroupListRequest("shop = 32", "ten", "nosuch"), GroupListRequest("shop = 33", "nosuch", "year"), GroupListRequest("shop = 33", None, "year"),
            GroupListRequest("shop = 33", "ten", "year", True, 0, 0), GroupListRequest("shop = 33", "ten", "year", True, 0, 1025), GroupListRequest("shop = 33", "ten", "year", True, 2 ** 31, 5),
            GroupListRequest("nosuch = 3", "ten", "year"), GroupListRequest("shop = 34", "genre", "ten", False, 3, 7)]
    got = e.list_groups(reqs)
    assert got[1].error and "syntax" in got[1].error.lower() and got[1].document_ids == [] and got[1].total == got[1].total_groups == 0
    assert got[2].error and "MATCHES" in got[2].error
    assert got[3].error and "nosuch" in got[3].error and got[4].error and "nosuch" in got[4].error and "group_by" in got[4].error
    assert got[5].error and "group_by" in got[5].error
    assert got[6].error and got[7].error and "limit" in got[6].error and got[8].error and "offset" in got[8].error
    for i in (0, 9, 10):
        gm.check(got[i], reqs[i])                                                  # an unknown field in the FILTER is null, as the filter VM has it
    assert got[0].total and got[10].total and got[9].total == got[9].total_groups == 0
    assert e.list_groups("shop = ", "ten", "year").error == got[1].error
    assert e.list_groups(None, None).error == got[5].error


def test_deletions_restore_and_a_replaced_group_column_invalidate(fx):
    e, lm, gm = fx
    s = Session(e)
    try:
        shop = lm.cols["shop"][0]
        reqs = [GroupListRequest(EVERYTHING, "shop", "uniq", True, 0, 1024), GroupListRequest(ONE_PCT, "wide", "rating", False, 0, 1024), GroupListRequest(None, "mid", None, True, 11000, 1024),
                GroupListRequest(LAST_ONLY, "shop", "shop", True, 0, 5), GroupListRequest(TWO_COLS, "ten", "wide", True, 0, 20)]
        before = run(s, gm, reqs, "live")
        assert s.list_groups(reqs) == before and s.last_group_list_stats()[:2] == (0, 4)
        heads = gm.heads(EVERYTHING, "shop", "uniq", True)[0]
        head_of_5 = int(heads[[int(shop[h]) for h in heads].index(5)])
        gone = sorted({head_of_5, D - 1} | set(range(3, D, 11)))                    # a head with other members behind it; the only member of shop 99
        try:
            assert e.delete_documents(gone) == len(gone)
            gm.set_deleted(gone)
            got = run(s, gm, reqs, "deleted")
            assert s.last_group_list_stats()[:2] == (4, 0)                          # the epoch moved: every mask is built again
            row = got[0].group_values.index("5")
            assert got[0].document_ids[row] != head_of_5 and shop[got[0].document_ids[row]] == 5       # the group's next member is its head now
            assert got[0].group_sizes[row] < before[0].group_sizes[before[0].group_values.index("5")]
            assert "99" in before[0].group_values and "99" not in got[0].group_values and got[0].total_groups == before[0].total_groups - 1      # the group vanished
            assert got[3].document_ids == [] and got[3].total_groups == 0 and got[3].total == 0
        finally:
            e.restore_documents(); gm.set_deleted([])
        assert run(s, gm, reqs, "restored") == before
        # a replaced group column changes the groups
        swap = np.asarray([d % 7 for d in range(D)], np.int64)
        e.set_column("swap", swap, facetable=False); gm.set_column("swap", swap)
        a = run(s, gm, [GroupListRequest(TWO_COLS, "swap", "rating", True, 0, 20)], "swap, seven groups")[0]
        swap = np.asarray([(d * 31) % 9000 for d in range(D)], np.int64)
        e.set_column("swap", swap, facetable=False); gm.set_column("swap", swap)
        b = run(s, gm, [GroupListRequest(TWO_COLS, "swap", "rating", True, 0, 20)], "swap, nine thousand groups")[0]
        assert a.total_groups == 7 and b.total_groups > 3000 and a.total == b.total
    finally:
        s.close()


@pytest.mark.parametrize("n", [12, 13, 14, 15, 17, 31])
def test_small_corpora_every_shape_of_the_partial_last_group(n):
    """Corpora of less than two groups of 16: the flags of the partial last group are read one by one.  The filters leave runs of accepted and refused
    documents that begin and end at every position of a group of four (1111 1000 0000: the first of a four alone refused)."""
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    shade = (["red", "blue", "green"] * 11)[:n]
    size = np.arange(1, n + 1, dtype=np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(n)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    lm = ListModel({"shade": (shade, True), "size": (size, False)}, list(range(100, 100 + n)))
    gm = GroupModel(lm)
    filters = ["size >= %d" % v for v in range(1, n + 2)] + ["size <= %d" % v for v in range(1, n)] + ["size = 5", "size = 6 OR size = 11", "size = 9 OR size >= 13", None]
    reqs = [GroupListRequest(x, g, c, asc, 0, 40) for x in filters for g, c, asc in (("shade", "size", True), ("size", "shade", False), ("shade", None, True))]
    got = run(e, gm, reqs, n)
    assert got[3 * 5].total == n - 5 and got[3 * 5].total_groups == 3 and sum(got[3 * 5].group_sizes) == n - 5      # size >= 6
    for x in filters:
        st = e.field_stats(x, "size", "shade")
        g = e.list_groups(x, "shade", "size", True, 0, 40)
        assert dict(zip(g.group_values, g.group_sizes)) == {grp.value: grp.count for grp in st.groups} and g.total == st.total, (n, x)


def test_duplicate_keys_in_different_groups_are_two_rows():
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    keys = [10, 11, 10, 12, 11, 10, 13, 12, 14, 13, 14, 15]
    shade = ["red", "blue", "blue", "red", "red", "green", "blue", "blue", "green", "green", "red", "blue"]
    size = np.asarray([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(k, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i, k in enumerate(keys)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    lm = ListModel({"shade": (shade, True), "size": (size, False)}, keys)
    gm = GroupModel(lm)
    reqs = [GroupListRequest(x, g, c, asc, off, 5) for x in (None, "shade = 'red'", "size >= 6") for g in ("shade", "size") for c in ("shade", "size", None) for asc in (True, False) for off in (0, 2)]
    run(e, gm, reqs, "duplicates")
    got = e.list_groups(None, "shade", "size", True, 0, 20)
    # documents 0 (red), 1 (blue) and 5 (green): key 10 heads two groups, each document its OWN shade
    assert got.document_ids == [10, 11, 10] and got.group_values == ["red", "blue", "green"] and got.values == ["1", "2", "6"] and got.group_sizes == [4, 5, 3]
    assert got.total_groups == 3 and got.total == 12
    assert e.delete_document_ids([0]) == 1
    gm.set_deleted([0])
    run(e, gm, reqs, "duplicates, document 0 deleted")
    got = e.list_groups(None, "shade", "size", True, 0, 20)
    assert got.document_ids == [11, 12, 10] and got.group_values == ["blue", "red", "green"] and got.group_sizes == [5, 3, 3] and got.total == 11
