"""top_groups on the GPU: a field's groups ranked by size, count, min, max, sum or mean and cut to a page, over the documents a filter accepts.

Expected rows come from numpy and Python on the columns' VALUES, as in test_gpu_field_stats.py (whose corpus this is: 4 099 documents, 256 walk groups of 16
and a partial last one, three of them deleted): membership by numpy comparisons, an int sum as a Python int, a double sum by math.fsum, the mean as
float(Fraction(exact sum) / count).  The order is a Python sorted over (has a figure, the figure or its negation, the value's text).  Every comparison is ==,
a NaN equal to a NaN.  Value columns: qty, big, price, four, infs and nanall (NaN for every member of tag group t5: a group with count == 0).  Group columns:
tag (7 values), one (1), g3000, uniq (every document its own value: more than 4096).  By slot size uniq's table lies in a workgroup's LDS (no field), in a
CU's whole LDS (one limb) and in global memory (four limbs)."""
import math
import re

import numpy as np
import pytest

from infidex_amd import Document, SearchEngine, StatsRequest, TopGroupsRequest
from infidex_amd.engine import Session
from tests.test_gpu_field_stats import D, FILTERS, Model, limbs, same

pytestmark = pytest.mark.gpu

BYS = ["size", "count", "min", "max", "sum", "mean"]
FIELDS = ["qty", "big", "price", "infs"]
GROUPS = ["tag", "g3000", "uniq"]


class TopModel(Model):
    def __init__(self):
        super().__init__()
        self.uniq = np.arange(D, dtype=np.int64) * 7 + 5
        self.nanall = np.round(np.random.default_rng(5).normal(3.0, 2.0, D), 1)
        self.nanall[np.arange(D) % 7 == 5] = np.nan
        self.live0 = self.live.copy()
        self.cache = {}; self.ranked = {}

    def members(self, x):
        extra = {"tag = 't5' OR num = 3": (self.tag == "t5") | (self.num == 3), "num < 20 AND idx >= 0": self.num < 20}
        if x in extra:
            return extra[x] & self.live
        if isinstance(x, str) and re.fullmatch(r"num = \d+", x):
            return (self.num == int(x[6:])) & self.live
        return super().members(x)

    def rows(self, x, g, field):
        """[(value, size, count, nan, min, max, sum, mean)] of every group of g with a member under filter x, in no order (the six figures None without a field)"""
        key = (x, g, field, self.live.tobytes())
        if key not in self.cache:
            live = self.members(x)
            gcol = getattr(self, g); ids = np.nonzero(live)[0]
            order = ids[np.argsort(gcol[ids], kind="stable")]
            cuts = np.nonzero(gcol[order][1:] != gcol[order][:-1])[0] + 1
            out = []
            for part in np.split(order, cuts) if len(order) else []:
                fig = self.figures(getattr(self, field)[part]) if field is not None else (None,) * 6
                out.append((str(gcol[part[0]]), len(part)) + tuple(fig))
            self.cache[key] = out
        return self.cache[key]

    def ranking(self, r):
        """the rows of request r's whole ranking, in order"""
        at = {"size": 1, "count": 2, "min": 4, "max": 5, "sum": 6, "mean": 7}[r.by]
        ck = (r.filter, r.group_by, r.field, r.by, bool(r.ascending), self.live.tobytes())
        if ck in self.ranked:
            return self.ranked[ck]

        def key(row):
            f = row[at]
            if f is None or (isinstance(f, float) and math.isnan(f)):
                return (1, 0, row[0])
            return (0, f if r.ascending else -f, row[0])
        self.ranked[ck] = sorted(self.rows(r.filter, r.group_by, r.field), key=key)
        return self.ranked[ck]

    def total(self, x):
        return int(self.members(x).sum())


def row_of(g):
    return (g.value, g.size, g.count, g.nan, g.min, g.max, g.sum, g.mean)


def rows_equal(got, want):
    return len(got) == len(want) and all(all(same(a, b) for a, b in zip(row_of(g), w)) for g, w in zip(got, want))


def check(m, got, r):
    """one answered request against the model"""
    want = m.ranking(r)
    assert got.error is None, (r, got.error)
    assert (got.total_groups, got.total) == (len(want), m.total(r.filter)), (r, got.total_groups, got.total, len(want))
    page = want[r.offset:r.offset + r.limit]
    assert rows_equal(got.groups, page), (r, [row_of(g) for g in got.groups][:3], page[:3])


def run(e, m, reqs):
    got = e.top_groups(reqs)
    assert len(got) == len(reqs)
    for g, r in zip(got, reqs):
        check(m, g, r)
    return got


def build(m):
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(int(k), "word%d item %d of the shelf" % (i % 11, i)) for i, k in enumerate(m.keys)])
    for name in ("idx", "num", "g3000", "uniq", "qty", "big", "price", "four", "infs", "wild", "nanall"):
        e.set_column(name, getattr(m, name), facetable=name == "num")
    e.set_column("tag", list(m.tag), facetable=True); e.set_column("one", list(m.one))
    assert e.delete_documents(m.keys[~m.live]) == 3
    return e


@pytest.fixture(scope="module")
def fx():
    m = TopModel()
    return build(m), m


def test_the_columns_are_what_the_cases_need():
    m = TopModel()
    assert len(np.unique(m.uniq)) == D > 4096 and len(np.unique(m.g3000)) == 3000 and len(np.unique(m.tag)) == 7 and len(np.unique(m.one)) == 1
    assert limbs(m.qty) == 1 and limbs(m.four) == 4 and limbs(m.price) == 3
    assert np.isnan(m.nanall[m.tag == "t5"]).all() and not np.isnan(m.nanall[m.tag != "t5"]).any()
    t3 = m.infs[(m.tag == "t3") & m.live]
    assert (t3 == np.inf).any() and (t3 == -np.inf).any()
    assert m.total("num = 1000") == 0 and m.total("idx = %d" % (D - 1)) == 1


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("g", GROUPS)
def test_every_ranking_in_pages_of_1024_and_of_7_is_the_model(fx, g, field):
    e, m = fx
    for x in FILTERS:
        n = len(m.rows(x, g, field))
        for lim in (1024, 7):
            reqs = [TopGroupsRequest(x, g, by, field, asc, off, lim) for by in BYS for asc in (True, False) for off in range(0, n + lim, lim)]
            got = run(e, m, reqs)
            per = len(reqs) // 12
            for k in range(12):                                   # the pages tile the ranking: every group once, the page behind the last one empty
                pages = got[k * per:(k + 1) * per]
                walked = [r.value for p in pages for r in p.groups]
                assert len(walked) == n == len(set(walked)) and pages[-1].groups == []


def test_the_three_placements_of_a_unique_column(fx):
    e, m = fx
    gv = len(np.unique(m.uniq))
    for field, want in ((None, (1, 0, 0)), ("qty", (0, 1, 0)), ("four", (0, 0, 1))):
        words = gv * (6 + 2 * limbs(getattr(m, field))) if field else gv
        assert want == ((1, 0, 0) if words <= 16384 else (0, 1, 0) if words <= 40960 else (0, 0, 1)), (field, words)
        for x in (None, "num < 20"):
            reqs = [TopGroupsRequest(x, "uniq", by, field, asc, 1500, 1024) for by in (BYS if field else ["size"]) for asc in (True, False)]
            run(e, m, reqs)
            assert e.last_top_groups_placement() == want and e.last_top_groups_stats()[2] == 1, (field, x)
    # a table of 3000 groups: where field_stats can answer too, and with four limbs in global memory as well
    run(e, m, [TopGroupsRequest("num < 20", "g3000", by, "four", True, 0, 1024) for by in BYS])
    assert e.last_top_groups_placement() == (0, 0, 1)


@pytest.mark.parametrize("g", ["tag", "g3000"])
def test_by_size_descending_is_field_stats_and_the_totals_are_the_listings(fx, g):
    e, m = fx
    for x in FILTERS:
        for field in FIELDS + ["four", "nanall"]:
            st = e.field_stats(x, field, g)
            n = len(st.groups)
            pages = e.top_groups([TopGroupsRequest(x, g, "size", field, False, off, 1024) for off in range(0, n + 1024, 1024)])
            rows = [r for p in pages for r in p.groups]
            assert len(rows) == n
            for r, s in zip(rows, st.groups):
                assert all(same(a, b) for a, b in zip(row_of(r), (s.value, s.count + s.nan, s.count, s.nan, s.min, s.max, s.sum, s.mean))), (x, field, r, s)
                assert repr(row_of(r)[2:]) == repr((s.count, s.nan, s.min, s.max, s.sum, s.mean))      # the same types and bytes
        t = e.top_groups(x, g)
        assert t.total_groups == e.list_groups(x, g).total_groups and t.total == e.list_documents(x).total


def test_ties_go_by_the_value_in_both_directions(fx):
    e, m = fx
    texts = sorted(str(v) for v in m.uniq[m.live])
    for asc in (True, False):
        for off in (0, 1, 1023, 1024, 2050, len(texts) - 1, len(texts)):
            got = e.top_groups(None, "uniq", "size", None, asc, off, 1024)
            assert [r.value for r in got.groups] == texts[off:off + 1024] and all(r.size == 1 and r.count is None and r.sum is None for r in got.groups)
            assert got.total_groups == got.total == len(texts)
        got = e.top_groups(None, "uniq", "count", "qty", asc, 2050, 7)
        assert [r.value for r in got.groups] == texts[2050:2057]
        for by, field in (("size", None), ("sum", "big"), ("mean", "price")):
            one = e.top_groups("num < 20", "one", by, field, asc, 0, 5)
            assert [r.value for r in one.groups] == ["only"] and one.total_groups == 1 and one.groups[0].size == one.total == m.total("num < 20")
            assert e.top_groups("num < 20", "one", by, field, asc, 1, 5).groups == []


def test_groups_without_a_figure_come_last_in_both_directions(fx):
    e, m = fx
    for asc in (True, False):
        for by in ("min", "max", "mean"):
            got = run(e, m, [TopGroupsRequest(None, "tag", by, "nanall", asc, 0, 20)])[0]
            assert [r.value for r in got.groups][-1] == "t5" and got.groups[-1].count == 0 and got.groups[-1].mean is None and got.groups[-1].nan == got.groups[-1].size
            figs = [getattr(r, by) for r in got.groups[:-1]]
            assert figs == sorted(figs, reverse=not asc)
        for by in ("sum", "count", "size"):                       # these have a figure at count == 0: the sum of nothing is 0.0
            got = run(e, m, [TopGroupsRequest(None, "tag", by, "nanall", asc, 0, 20)])[0]
            assert len(got.groups) == 7
        for by in ("sum", "mean"):
            got = run(e, m, [TopGroupsRequest(None, "tag", by, "infs", asc, 0, 20)])[0]
            assert got.groups[-1].value == "t3" and math.isnan(getattr(got.groups[-1], by))
            ends = (got.groups[0], got.groups[-2])
            assert {getattr(r, by) for r in ends} == {np.inf, -np.inf} and getattr(ends[0], by) == (-np.inf if asc else np.inf)
        # several groups without a figure: among themselves by value
        got = run(e, m, [TopGroupsRequest("tag = 't5' OR num = 3", "g3000", "max", "nanall", asc, 0, 1024)])[0]
        tail = [r.value for r in got.groups if r.max is None]
        assert len(tail) > 100 and tail == sorted(tail) and [r.value for r in got.groups][-len(tail):] == tail


def test_the_same_bytes_alone_among_sixteen_on_two_sessions_and_at_any_digit_width(fx):
    e, m = fx
    s, t = Session(e), Session(e)
    try:
        for probe in (TopGroupsRequest("num < 20", "g3000", "sum", "price", False, 300, 1024), TopGroupsRequest(None, "uniq", "mean", "big", True, 4000, 200),
                      TopGroupsRequest("num < 20", "uniq", "size", None, False, 5, 64)):
            alone = s.top_groups([probe])[0]
            check(m, alone, probe)
            others = [TopGroupsRequest(["num < 20", None, "tag = 't1'"][i % 3], GROUPS[i % 3], BYS[i % 6], FIELDS[i % 4], i % 2 == 0, 3 * i, 40 + i) for i in range(15)]
            for at in (0, 7, 15):
                among = s.top_groups(others[:at] + [probe] + others[at:])
                assert repr(among[at]) == repr(alone)
            assert repr(t.top_groups([probe])[0]) == repr(alone)
            for bits in (4, 11):
                s.set_list_digit_bits(bits)
                assert repr(s.top_groups([probe])[0]) == repr(alone), bits
                assert repr(s.top_groups(others)) == repr(t.top_groups(others))
    finally:
        s.close(); t.close()


def test_accumulate_passes_and_masks_are_shared(fx):
    e, m = fx
    s = Session(e)
    try:
        x = "num < 20 AND idx >= 0"                                 # (a filter no other test has built a mask of on this session)
        sixteen = [TopGroupsRequest(x, "g3000", BYS[i % 6], "price", i % 2 == 0, 40 * (i // 6), 40) for i in range(16)]
        run(s, m, sixteen)
        built, reused, acc, passes, launches = s.last_top_groups_stats()
        assert (built, reused, acc) == (1, 0, 1)                  # sixteen pages, directions and bys of one table: ONE walk over the documents
        assert passes == 9 and launches == 1 + 1 + 1 + 2 * 9 + 2  # the widest composite (a double sum: 98 bits) at 11 bits; mask build, accumulate, keys, hist + pick per pass, gather, page
        run(s, m, sixteen[:3] + [TopGroupsRequest(x, "g3000", "sum", "qty"), TopGroupsRequest(x, "tag", "sum", "price"), TopGroupsRequest(x, "g3000")])
        assert s.last_top_groups_stats()[:3] == (0, 1, 4)         # another field, another group column and no field are tables of their own
        run(s, m, [TopGroupsRequest(None, "tag")])
        assert s.last_top_groups_stats()[:3] == (0, 0, 1)         # the index's Deleted flags, no mask
        seventeen = [TopGroupsRequest("num = %d" % i, "tag", "mean", "qty") for i in range(17)]      # Python splits: 16 + 1
        got = run(s, m, seventeen)
        assert len(got) == 17 and all(p.total_groups for p in got) and s.last_top_groups_stats()[:3] == (1, 0, 1)
        assert s.list_documents("num = 16").total == got[16].total and s.last_list_stats()[:2] == (0, 1)      # the mask serves list_documents
    finally:
        s.close()


def test_refusals_are_per_request_at_any_position(fx):
    e, m = fx
    good = [TopGroupsRequest("num < 20", "tag", "sum", "price", False, 0, 5), TopGroupsRequest(None, "g3000", "max", "qty", True, 7, 9), TopGroupsRequest("tag = 't1'", "uniq")]
    bad = [(TopGroupsRequest("num = ", "tag"), "syntax"), (TopGroupsRequest("tag MATCHES 't[12]'", "tag"), "MATCHES"), (TopGroupsRequest(None, None), "group_by"),
           (TopGroupsRequest(None, "nosuch"), "nosuch"), (TopGroupsRequest(None, "tag", "median", "qty"), "median"), (TopGroupsRequest(None, "tag", "sum"), "needs a field"),
           (TopGroupsRequest(None, "tag", "sum", "nosuch"), "nosuch"), (TopGroupsRequest(None, "tag", "min", "tag"), "string"),
           (TopGroupsRequest(None, "tag", "sum", "wild"), "128 binary digits"), (TopGroupsRequest(None, "tag", "size", None, False, 0, 0), "limit"),
           (TopGroupsRequest(None, "tag", "size", None, False, 0, 1025), "limit"), (TopGroupsRequest(None, "tag", "size", None, False, 2 ** 31, 5), "offset")]
    alone = {id(r): e.top_groups([r])[0] for r in good + [b for b, _ in bad]}
    for b, word in bad:
        a = alone[id(b)]
        assert a.error and word.lower() in a.error.lower() and a.groups == [] and a.total == a.total_groups == 0, (b, a.error)
    for g in good:
        check(m, alone[id(g)], g)
    # a call of sixteen: refused requests first, in the middle and last, between answered ones — each what it is alone
    call = [bad[0][0], good[0], good[1], bad[1][0], bad[2][0], good[2], bad[3][0], bad[4][0], good[0], bad[5][0], bad[6][0], good[1], bad[7][0], bad[8][0], good[2], bad[9][0]]
    assert len(call) == 16
    got = e.top_groups(call)
    assert [repr(a) for a in got] == [repr(alone[id(r)]) for r in call]
    assert e.top_groups("num = ", "tag").error == alone[id(bad[0][0])].error


@pytest.mark.parametrize("n", [12, 13, 14, 15, 17, 31])
def test_small_corpora_every_shape_of_the_partial_last_group(n):
    """Corpora of less than two groups of 16: the flags of the partial last group are read one by one.  The filters leave runs of accepted and refused
    documents that begin and end at every position of a group of four."""
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    shade = (["red", "blue", "green"] * 11)[:n]
    size = np.arange(1, n + 1, dtype=np.int64)
    half = size * 0.5 - 3.0
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(n)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False); e.set_column("half", half, facetable=False)
    filters = ["size >= %d" % v for v in range(1, n + 2)] + ["size <= %d" % v for v in range(1, n)] + ["size = 5", "size = 6 OR size = 11", "size = 9 OR size >= 13", None]
    for x in filters:
        st = e.field_stats(x, "half", "shade")
        got = e.top_groups([TopGroupsRequest(x, "shade", "size", "half", False, 0, 40), TopGroupsRequest(x, "shade", "sum", "half", True, 0, 40),
                            TopGroupsRequest(x, "size", "size", None, False, 0, 40), TopGroupsRequest(x, "size", "mean", "half", False, 0, 40)])
        assert all(g.error is None and g.total == st.total for g in got), (n, x)
        assert [(r.value, r.count, r.sum, r.mean, r.min, r.max) for r in got[0].groups] == [(s.value, s.count, s.sum, s.mean, s.min, s.max) for s in st.groups], (n, x)
        assert sorted((r.sum, r.value) for r in got[1].groups) == [(r.sum, r.value) for r in got[1].groups] and len(got[1].groups) == len(st.groups)
        members = sorted(str(int(v)) for v in size if st.total and _accepts(x, int(v)))
        assert [r.value for r in got[2].groups] == members and got[2].total_groups == st.total == len(members), (n, x)
        assert [r.mean for r in got[3].groups] == sorted((float(v) * 0.5 - 3.0 for v in members), reverse=True)


def _accepts(x, v):
    """the small corpora's filters on a value of `size`"""
    if x is None:
        return True
    return eval(x.replace("size", str(v)).replace(" = ", " == ").replace("OR", "or"))


def test_deletions_and_a_restore_follow_the_model(fx):
    e, m = fx
    s = Session(e)
    try:
        reqs = [TopGroupsRequest(None, "tag", "sum", "big", False, 0, 20), TopGroupsRequest("num < 20", "g3000", "mean", "price", True, 100, 1024),
                TopGroupsRequest(None, "uniq", "max", "qty", False, 3000, 1024), TopGroupsRequest("idx = %d" % (D - 1), "uniq", "size", None, False, 0, 5)]
        before = run(s, m, reqs)
        assert s.top_groups(reqs) == before and s.last_top_groups_stats()[:2] == (0, 2)
        gone = sorted({D - 1} | set(range(3, D, 11)))
        try:
            assert e.delete_documents(m.keys[gone]) == len([d for d in gone if m.live[d]])
            m.live = m.live0.copy(); m.live[gone] = False
            got = run(s, m, reqs)
            assert s.last_top_groups_stats()[:2] == (2, 0)        # the epoch moved: every mask is built again
            assert got[0].total == before[0].total - len([d for d in gone if m.live0[d]]) and got[3].groups == [] and got[3].total_groups == 0
            assert got[2].total_groups == got[2].total < before[2].total_groups
        finally:
            e.restore_documents(); m.live = np.ones(D, bool)
        after = run(s, m, reqs)                                     # everything lives: the three documents deleted at the start too
        assert after[0].total == D and after[2].total_groups == D
        assert e.delete_documents(m.keys[~m.live0]) == 3
        m.live = m.live0.copy()
        assert run(s, m, reqs) == before
    finally:
        m.live = m.live0.copy()
        s.close()
