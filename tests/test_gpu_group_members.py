"""SearchEngine.list_group_members on the GPU: list_groups' rows, each with the first per_group members of its group in list_documents' order.

The expected answer is a test-side model on top of tests/test_gpu_list_groups.py's GroupModel and tests/test_gpu_list_documents.py's ListModel: the groups of a
page are GroupModel.page(r)'s rows, and along ListModel.order(filter, order_by, ascending) — every accepted live document in the listing's order — the members
of a group are the first per_group occurrences of that group.  Every comparison is exact equality of DocumentKeys, value texts, group texts, sizes and totals.
The corpus, the columns and the filters are those modules' (70 001 documents: no multiple of 16)."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, GroupListRequest, GroupMembersRequest, GroupMembersListing, GroupMembers, ListRequest
from infidex_amd.engine import Session
from tests.browse_model import facet_text
from tests.test_gpu_list_documents import ListModel, D, ONE_PCT, NOTHING, EVERYTHING, LAST_ONLY, TWO_COLS, FILTERS, variant
from tests.test_gpu_list_groups import GroupModel, GROUPS, ORDERS, fx      # noqa: F401 (fx: the module's fixture, built once for this module too)

pytestmark = pytest.mark.gpu

PER_GROUP = [1, 2, 3, 16]


def groups_request(r):
    return GroupListRequest(r.filter, r.group_by, r.order_by, r.ascending, r.offset, r.limit)


class MembersModel:
    def __init__(self, gm):
        self.gm, self.lm = gm, gm.lm
        self._by = {}

    def set_deleted(self, ids):
        self.gm.set_deleted(ids); self._by = {}

    def set_column(self, name, vals):
        self.gm.set_column(name, vals); self._by = {}

    def by_group(self, x, g, c, asc):
        """(the set's documents by group number, within a group in the listing's order; their group numbers, ascending)"""
        k = (x, g, c, bool(asc))
        if k not in self._by:
            o = self.lm.order(x, c, asc)
            go = self.gm.gid(g)[0][o]
            so = np.argsort(go, kind="stable")
            self._by = {k: (o[so], go[so])}                                   # (the last listing only: its pages follow one another)
        return self._by[k]

    def page(self, r):
        rows = self.gm.page(groups_request(r))
        heads = self.gm.heads(r.filter, r.group_by, r.order_by, r.ascending)[0][r.offset:r.offset + r.limit]
        ids = self.gm.gid(r.group_by)[0]
        docs, gs = self.by_group(r.filter, r.group_by, r.order_by, r.ascending)
        out = []
        for j, h in enumerate(heads):
            lo = int(np.searchsorted(gs, ids[h], "left"))
            mem = docs[lo:lo + min(r.per_group, rows.group_sizes[j])]
            assert mem[0] == h
            vals = [] if r.order_by is None else [facet_text(self.lm.cols[r.order_by][0][i]) for i in mem]
            out.append(GroupMembers(rows.group_values[j], rows.group_sizes[j], [int(k) for k in self.lm.keys[mem]], vals))
        return GroupMembersListing(out, rows.total_groups, rows.total, None)

    def check(self, got, r, ctx=None):
        want = self.page(r)
        assert got.error is None, (ctx, r, got.error)
        assert (got.total_groups, got.total) == (want.total_groups, want.total), (ctx, r, got.total_groups, got.total, want.total_groups, want.total)
        assert len(got.groups) == len(want.groups), (ctx, r, len(got.groups), len(want.groups))
        for j, (g, w) in enumerate(zip(got.groups, want.groups)):
            assert g == w, (ctx, r, j, g, w)


def run(s, mm, reqs, ctx=None):
    """asks reqs sixteen at a time of session (or engine) s and holds every answer to the model"""
    got = s.list_group_members(reqs)
    assert len(got) == len(reqs)
    for g, r in zip(got, reqs):
        mm.check(g, r, ctx)
    return got


def as_group_listing(m):
    """what list_groups returns for the request a GroupMembersListing answers: every group's head"""
    return ([g.document_ids[0] for g in m.groups], [g.values[0] for g in m.groups if g.values], [g.group_value for g in m.groups], [g.size for g in m.groups],
            m.total_groups, m.total, m.error)


@pytest.fixture(scope="module")
def mx(fx):
    e, lm, gm = fx
    return e, lm, MembersModel(gm)


@pytest.mark.parametrize("g", GROUPS)
def test_every_group_column_order_filter_direction_and_per_group(mx, g):
    """Every order, filter and direction; pages at offset 0, in the middle, a short last page and offset == total_groups; per_group 1, 2, 3 and 16 rotate
    over the pages so that every (order, filter) meets each of them and every kind of page meets each across the filters and directions."""
    e, lm, mm = mx
    s = Session(e)
    try:
        for c in ORDERS:
            reqs, seen = [], set()
            for fi, x in enumerate(FILTERS):
                for asc in (True, False):
                    tg = len(mm.gm.heads(x, g, c, asc)[0])
                    for p, (off, lim) in enumerate(((0, 20), (tg // 2, 65), (max(tg - 30, 0), 97), (tg, 20))):
                        per = PER_GROUP[(p + fi + (0 if asc else 1)) % 4]
                        seen.add((p, per))
                        reqs.append(GroupMembersRequest(x, g, c, asc, per, off, lim))
            assert len(seen) == 16
            got = run(s, mm, reqs, (g, c))
            heads = s.list_groups([groups_request(r) for r in reqs])
            for m, h in zip(got, heads):                                      # heads, sizes and totals are list_groups'
                assert as_group_listing(m) == (h.document_ids, h.values, h.group_values, h.group_sizes, h.total_groups, h.total, h.error)
            for k, x in enumerate(FILTERS):
                first = got[8 * k]
                if x == NOTHING:
                    assert first.total_groups == first.total == 0 and first.groups == [] and first.error is None
                if x == LAST_ONLY:
                    assert [grp.document_ids for grp in first.groups] == [[D - 1]] and first.groups[0].size == 1 and first.total_groups == first.total == 1
    finally:
        s.close()


def test_one_member_per_group_is_list_groups_field_for_field(mx):
    e, lm, mm = mx
    reqs = [GroupMembersRequest(x, g, c, asc, 1, off, 1024) for x, g, c, asc, off in ((TWO_COLS, "mid", "wide", False, 2000), (None, "shop", "rating", True, 0), (EVERYTHING, "ten", None, True, 0),
                                                                                 (ONE_PCT, "wide", "genre", False, 5), (None, "uniq", "uniq", False, 69000), (NOTHING, "shop", "ten", True, 0))]
    got = run(e, mm, reqs, "one per group")
    want = e.list_groups([groups_request(r) for r in reqs])
    for m, h in zip(got, want):
        assert all(len(g.document_ids) == 1 for g in m.groups)
        assert as_group_listing(m) == (h.document_ids, h.values, h.group_values, h.group_sizes, h.total_groups, h.total, h.error)


@pytest.mark.parametrize("c,asc", [("rating", True), (None, False), ("ten", False)])
def test_a_groups_members_are_list_documents_of_that_group(mx, c, asc):
    e, lm, mm = mx
    s = Session(e)
    try:
        for x in FILTERS:
            m = s.list_group_members(x, "shop", c, asc, 3, 0, 1024)
            assert m.error is None
            want = s.list_documents([ListRequest("shop = %s" % g.group_value if x is None else "(%s) AND shop = %s" % (x, g.group_value), c, asc, 0, 3) for g in m.groups])
            for g, w in zip(m.groups, want):
                assert w.error is None and (g.document_ids, g.values, g.size) == (w.document_ids, w.values, w.total), (x, g.group_value)
            assert len(m.groups) == m.total_groups and sum(g.size for g in m.groups) == m.total
    finally:
        s.close()


def test_members_under_ties_are_the_lowest_indices_in_both_directions(mx):
    e, lm, mm = mx
    shop = lm.cols["shop"][0]
    for c in ("one", None):                                                   # a constant key, no key: the order is the index order whatever the direction
        for asc in (True, False):
            m = e.list_group_members(EVERYTHING, "shop", c, asc, 16, 0, 100)
            assert m.error is None and m.total_groups == 100
            for g in m.groups:
                mem = np.nonzero(shop == int(g.group_value))[0]
                assert g.document_ids == [int(d) for d in mem[:16]] and g.size == len(mem), (c, asc, g.group_value)      # (keys are indices here)
            mm.check(m, GroupMembersRequest(EVERYTHING, "shop", c, asc, 16, 0, 100))
    # ties at the best key: shop's members ordered by ten, some 70 per key
    for asc in (True, False):
        run(e, mm, [GroupMembersRequest(EVERYTHING, "shop", "ten", asc, 16, 0, 100)], "ties")


def test_short_groups_carry_what_they_have(mx):
    e, lm, mm = mx
    m = run(e, mm, [GroupMembersRequest(TWO_COLS, "uniq", "rating", False, 16, 100, 256)], "uniq")[0]
    assert len(m.groups) == 256 and all(len(g.document_ids) == 1 and g.size == 1 for g in m.groups)
    m = run(e, mm, [GroupMembersRequest("shop = 99", "shop", "year", True, 16, 0, 20)], "shop 99")[0]
    assert [(g.group_value, g.size, g.document_ids) for g in m.groups] == [("99", 1, [D - 1])]
    # groups of exactly per_group members, one fewer and one more: found through the model among mid's groups under TWO_COLS
    sizes = mm.gm.heads(TWO_COLS, "mid", "rating", True)[1]
    for per in (2, 3):
        assert all((sizes == k).any() for k in (per - 1, per, per + 1))
    tg = len(mm.gm.heads(TWO_COLS, "mid", "rating", True)[0])
    for per in (2, 3):
        pages = run(e, mm, [GroupMembersRequest(TWO_COLS, "mid", "rating", True, per, off, 1024) for off in range(0, tg, 1024)], "short")
        assert all(len(g.document_ids) == min(g.size, per) for p in pages for g in p.groups)
        assert {per - 1, per, per + 1} <= {g.size for p in pages for g in p.groups}


def test_one_group_takes_every_member_into_one_row(mx):
    e, lm, mm = mx
    for c, asc in ((None, True), ("ten", True), ("uniq", False), ("rating", False)):
        m = run(e, mm, [GroupMembersRequest(EVERYTHING, "one", c, asc, 16, 0, 20)], "contention")[0]
        w = e.list_documents(EVERYTHING, c, asc, 0, 16)
        assert len(m.groups) == 1 and m.groups[0].size == D == m.total and (m.groups[0].document_ids, m.groups[0].values) == (w.document_ids, w.values)


def test_sixteen_full_pages_of_one_listing_take_four_member_walks(mx):
    e, lm, mm = mx
    s = Session(e)
    try:
        reqs = [GroupMembersRequest(None, "mid", "wide", i % 2 == 0, 4, 650 * i, 1024) for i in range(16)]      # two specs of eight requests, 10 240 LDS words each
        run(s, mm, reqs, "packing")
        built, reused, heads, hist, walks, launches = s.last_group_members_stats()
        assert (built, reused, heads) == (0, 0, 2) and walks >= 4
        reqs = [GroupMembersRequest(TWO_COLS, "mid", "rating", True, 4, 700 * i, 1024) for i in range(16)]      # one spec: 163 840 words, four times the LDS of a CU
        run(s, mm, reqs, "packing, one spec")
        built, reused, heads, hist, walks, launches = s.last_group_members_stats()
        assert (built, reused, heads) == (1, 0, 1) and 4 <= walks <= 16
        assert launches == 1 + 2 + 16 * 6 + 1 + walks + 1   # mask build; heads, heads mask; per page hist, pick, count, prefix, gather, sort; page codes; walks; member rows
        small = [GroupMembersRequest(TWO_COLS, "mid", "rating", True, 3, 40 * i, 40) for i in range(16)]
        run(s, mm, small, "sixteen small pages")
        assert s.last_group_members_stats()[:5] == (0, 1, 1, 16, 1)          # sixteen small pages share one walk
    finally:
        s.close()


def test_the_same_bytes_alone_among_sixteen_on_two_sessions_and_at_any_digit_width(mx):
    e, lm, mm = mx
    s, t = Session(e), Session(e)
    try:
        probe = GroupMembersRequest(TWO_COLS, "mid", "wide", False, 3, 2000, 1024)
        alone = s.list_group_members([probe])[0]
        mm.check(alone, probe)
        others = [GroupMembersRequest([ONE_PCT, None, EVERYTHING][i % 3], GROUPS[i % 8], ORDERS[i % 6], i % 2 == 0, PER_GROUP[i % 4], 3 * i, 40 + i) for i in range(15)]
        for at in (0, 7, 15):
            among = run(s, mm, others[:at] + [probe] + others[at:], at)
            assert repr(among[at]) == repr(alone)
        assert repr(t.list_group_members([probe])[0]) == repr(alone)
        for bits in (4, 11):
            s.set_list_digit_bits(bits)
            assert repr(s.list_group_members([probe])[0]) == repr(alone), bits
            assert repr(run(s, mm, others, bits)) == repr(t.list_group_members(others))
    finally:
        s.close(); t.close()


def test_refusals_are_per_request(mx):
    e, lm, mm = mx
    R = GroupMembersRequest
    reqs = [R("shop = 31", "ten", "year"), R("shop = ", "ten", "year"), R("ten MATCHES 'c[12]'", "ten", "year"), R("shop = 32", "ten", "nosuch"), R("shop = 33", "nosuch", "year"),
            R("shop = 33", None, "year"), R("shop = 33", "ten", "year", True, 3, 0, 0), R("shop = 33", "ten", "year", True, 3, 0, 1025), R("shop = 33", "ten", "year", True, 3, 2 ** 31, 5),
            R("shop = 33", "ten", "year", True, 0), R("shop = 33", "ten", "year", True, 17), R("shop = 33", "ten", "year", True, 17, 0, 241), R("shop = 33", "ten", "year", True, 5, 0, 1024),
            R("nosuch = 3", "ten", "year"), R("shop = 34", "genre", "ten", False, 16, 3, 256), R("shop = 35", "ten", "year", True, 4, 0, 1024)]
    got = e.list_group_members(reqs)
    assert got[1].error and "syntax" in got[1].error.lower() and got[1].groups == [] and got[1].total == got[1].total_groups == 0
    assert got[2].error and "MATCHES" in got[2].error
    assert got[3].error and "nosuch" in got[3].error and got[4].error and "nosuch" in got[4].error and "group_by" in got[4].error
    assert got[5].error and "group_by" in got[5].error
    assert got[6].error and got[7].error and "limit" in got[6].error and got[8].error and "offset" in got[8].error
    assert got[9].error and "per_group" in got[9].error and got[10].error and "per_group" in got[10].error
    assert got[11].error and "per_group" in got[11].error and got[12].error and "4096" in got[12].error
    for i in (0, 13, 14, 15):
        mm.check(got[i], reqs[i])                                             # an unknown field in the FILTER is null, as the filter VM has it
    assert got[0].total and got[14].total and got[15].total and got[13].total == got[13].total_groups == 0
    assert e.list_group_members("shop = ", "ten", "year").error == got[1].error
    assert e.list_group_members(None, None).error == got[5].error
    assert e.list_group_members(None, "ten", per_group=0).error == got[9].error


def test_deletions_restore_and_a_replaced_group_column_invalidate(mx):
    e, lm, mm = mx
    s = Session(e)
    try:
        shop = lm.cols["shop"][0]
        reqs = [GroupMembersRequest(EVERYTHING, "shop", "uniq", True, 3, 0, 1024), GroupMembersRequest(ONE_PCT, "wide", "rating", False, 2, 0, 1024),
                GroupMembersRequest(None, "mid", None, True, 4, 11000, 1024), GroupMembersRequest(LAST_ONLY, "shop", "shop", True, 16, 0, 5), GroupMembersRequest(TWO_COLS, "ten", "wide", True, 16, 0, 20)]
        before = run(s, mm, reqs, "live")
        assert s.list_group_members(reqs) == before and s.last_group_members_stats()[:2] == (0, 4)
        row = [g.group_value for g in before[0].groups].index("5")
        second_of_5 = before[0].groups[row].document_ids[1]                    # (keys are indices here)
        gone = sorted({second_of_5, D - 1} | set(range(3, D, 11)))              # a member behind its head; the only member of shop 99
        try:
            assert e.delete_documents(gone) == len(gone)
            mm.set_deleted(gone)
            got = run(s, mm, reqs, "deleted")
            assert s.last_group_members_stats()[:2] == (4, 0)                  # the epoch moved: every mask is built again
            row2 = [g.group_value for g in got[0].groups].index("5")
            assert second_of_5 not in got[0].groups[row2].document_ids and all(shop[d] == 5 for d in got[0].groups[row2].document_ids) and len(got[0].groups[row2].document_ids) == 3
            assert got[0].groups[row2].size < before[0].groups[row].size
            assert "99" not in [g.group_value for g in got[0].groups] and got[0].total_groups == before[0].total_groups - 1
            assert got[3].groups == [] and got[3].total_groups == 0 and got[3].total == 0
        finally:
            e.restore_documents(); mm.set_deleted([])
        assert run(s, mm, reqs, "restored") == before
        # a replaced group column changes the groups
        swap = np.asarray([d % 7 for d in range(D)], np.int64)
        e.set_column("swap", swap, facetable=False); mm.set_column("swap", swap)
        a = run(s, mm, [GroupMembersRequest(TWO_COLS, "swap", "rating", True, 3, 0, 20)], "swap, seven groups")[0]
        swap = np.asarray([(d * 31) % 9000 for d in range(D)], np.int64)
        e.set_column("swap", swap, facetable=False); mm.set_column("swap", swap)
        b = run(s, mm, [GroupMembersRequest(TWO_COLS, "swap", "rating", True, 3, 0, 20)], "swap, nine thousand groups")[0]
        assert a.total_groups == 7 and b.total_groups > 3000 and a.total == b.total
    finally:
        s.close()


@pytest.mark.parametrize("n", [12, 13, 14, 15, 17, 31])
def test_small_corpora_every_shape_of_the_partial_last_group(n):
    """Corpora of less than two groups of 16: the flags of the partial last group are read one by one.  The filters leave runs of accepted and refused
    documents that begin and end at every position of a group of four."""
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    shade = (["red", "blue", "green"] * 11)[:n]
    size = np.arange(1, n + 1, dtype=np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(n)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    mm = MembersModel(GroupModel(ListModel({"shade": (shade, True), "size": (size, False)}, list(range(100, 100 + n)))))
    filters = ["size >= %d" % v for v in range(1, n + 2)] + ["size <= %d" % v for v in range(1, n)] + ["size = 5", "size = 6 OR size = 11", "size = 9 OR size >= 13", None]
    reqs = [GroupMembersRequest(x, g, c, asc, PER_GROUP[(i + j) % 4], 0, 40) for i, x in enumerate(filters)
            for j, (g, c, asc) in enumerate((("shade", "size", True), ("size", "shade", False), ("shade", None, True), ("shade", "size", False)))]
    got = run(e, mm, reqs, n)
    assert got[4 * 5].total == n - 5 and got[4 * 5].total_groups == 3 and sum(g.size for g in got[4 * 5].groups) == n - 5      # size >= 6
    whole = e.list_group_members(None, "shade", "size", True, 16, 0, 40)
    assert sorted(d for g in whole.groups for d in g.document_ids) == list(range(100, 100 + n))     # every document is a member of its shade


def test_documents_with_duplicate_keys_are_members_of_their_own():
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    keys = [10, 11, 10, 12, 11, 10, 13, 12, 14, 13, 14, 15]
    shade = ["red", "blue", "blue", "red", "red", "green", "blue", "blue", "green", "green", "red", "blue"]
    size = np.asarray([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(k, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i, k in enumerate(keys)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    mm = MembersModel(GroupModel(ListModel({"shade": (shade, True), "size": (size, False)}, keys)))
    reqs = [GroupMembersRequest(x, g, c, asc, per, off, 5) for x in (None, "shade = 'red'", "size >= 6") for g in ("shade", "size") for c in ("shade", "size", None) for asc in (True, False)
            for per, off in ((1, 0), (2, 2), (3, 0), (16, 0))]
    run(e, mm, reqs, "duplicates")
    got = e.list_group_members(None, "shade", "size", True, 3, 0, 20)
    # red: documents 0, 3, 4; blue: 1, 2, 6; green: 5, 8, 9 — key 10 is a member of all three groups, each document under its OWN shade
    assert [(g.group_value, g.size, g.document_ids, g.values) for g in got.groups] == \
        [("red", 4, [10, 12, 11], ["1", "4", "5"]), ("blue", 5, [11, 10, 13], ["2", "3", "7"]), ("green", 3, [10, 14, 13], ["6", "9", "10"])]
    assert got.total_groups == 3 and got.total == 12
    assert e.delete_document_ids([0]) == 1
    mm.set_deleted([0])
    run(e, mm, reqs, "duplicates, document 0 deleted")
    got = e.list_group_members(None, "shade", "size", False, 2, 0, 20)
    assert [(g.group_value, g.document_ids) for g in got.groups] == [("blue", [15, 12]), ("red", [14, 11]), ("green", [13, 14])] and got.total == 11
