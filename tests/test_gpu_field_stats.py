"""field_stats on the GPU: counts, NaNs, min / max and the EXACT sum and mean of a numeric field over the documents a filter accepts, whole and per group.

Expected values come from numpy on the columns' VALUES: membership by numpy comparisons, the sum of an int column as a Python int, the sum of a double
column by math.fsum (the exact real sum rounded once), the mean as float(Fraction(exact sum) / count).  Every comparison is ==.
4 099 documents: 256 walk groups of 16 and a partial last one of three; three of them deleted.  Value columns: qty (small int64), big (int64 with both
extremes: the sum exceeds 64 bits), price (doubles of three limbs with NaNs, +-0.0, 2^-20 and values near +-1e11: a float addition in any order misses
the exact sum), four (doubles of four limbs), infs (+inf in some tag groups, -inf in others, both in one), wild (1e-30 and 1e30: refused).  Group columns:
tag (7 strings), one (a single value), g1000 and g3000 (ints; by size their slots are in a workgroup's LDS, in a CU's whole LDS or in global memory, depending on
the field's limbs and on the call), qty by itself."""
import math
from fractions import Fraction

import numpy as np
import pytest

from infidex_amd import Document, ListRequest, SearchEngine, StatsRequest
from infidex_amd.engine import Session

pytestmark = pytest.mark.gpu

D = 4099
I64 = np.iinfo(np.int64)
FILTERS = [None, "num = 3", "num = 1000", "num >= 0", "idx = %d" % (D - 1), "num >= 30 AND tag = 't1'"]
FIELDS = ["qty", "big", "price", "four", "infs"]


def limbs(col):
    """the number of 32-bit limbs exact_sum.h needs for the finite non-zero values of col"""
    lo = hi = None
    for v in np.unique(col[np.isfinite(col) & (col != 0)] if col.dtype.kind == "f" else col[col != 0]):
        fr = abs(Fraction(float(v)) if col.dtype.kind == "f" else Fraction(int(v)))
        l = -(fr.denominator.bit_length() - 1) if fr.denominator > 1 else (fr.numerator & -fr.numerator).bit_length() - 1
        h = fr.numerator.bit_length() - fr.denominator.bit_length()
        h = h if Fraction(2) ** h <= fr else h - 1
        if col.dtype.kind != "f":
            l = 0
        lo = l if lo is None else min(lo, l); hi = h if hi is None else max(hi, h)
    return (1 + hi - lo + 31) // 32


class Model:
    def __init__(self):
        rng = np.random.default_rng(11)
        self.keys = np.arange(D, dtype=np.int64) * 3 + 1000
        self.idx = np.arange(D, dtype=np.int64)
        self.num = rng.integers(0, 100, D).astype(np.int64)
        self.tag = np.array(["t%d" % (i % 7) for i in range(D)])
        self.one = np.array(["only"] * D)
        self.g1000 = (rng.permutation(D) % 1000).astype(np.int64)
        self.g3000 = (rng.permutation(D) % 3000).astype(np.int64)
        self.qty = rng.integers(-5, 40, D).astype(np.int64)
        self.big = rng.integers(-2 ** 62, 2 ** 62, D).astype(np.int64)
        self.big[rng.choice(D, 200, replace=False)] = I64.max; self.big[rng.choice(D, 90, replace=False)] = I64.min; self.big[D - 1] = I64.max
        self.price = np.round(rng.normal(50.0, 30.0, D), 2)
        pick = rng.choice(D - 1, 163, replace=False)
        self.price[pick[:60]] *= 1e9; self.price[pick[60:120]] *= -1e9; self.price[pick[120:160]] = np.nan
        self.price[pick[160]] = -0.0; self.price[pick[161]] = 0.0; self.price[pick[162]] = 2.0 ** -20; self.price[D - 1] = 12.25
        self.four = rng.integers(1, 1000, D) * 2.0 ** -50 * rng.choice([1.0, -1.0], D)
        big4 = rng.choice(D, 300, replace=False); self.four[big4] = rng.integers(1, 1000, 300) * 2.0 ** 60 * rng.choice([1.0, -1.0], 300)
        self.infs = np.round(rng.normal(0.0, 5.0, D), 1)
        t = np.arange(D) % 7
        self.infs[np.nonzero(t == 1)[0][::40]] = np.inf; self.infs[np.nonzero(t == 2)[0][::50]] = -np.inf
        self.infs[np.nonzero(t == 3)[0][::60]] = np.inf; self.infs[np.nonzero(t == 3)[0][1::60]] = -np.inf; self.infs[np.nonzero(t == 4)[0][::30]] = np.nan
        self.wild = np.where(np.arange(D) % 2 == 0, 1e-30, 1e30)
        self.live = np.ones(D, bool); self.live[[0, 2048, D - 2]] = False

    def members(self, x):
        """bool per document: live and accepted by filter x (the comparisons the tests use)"""
        acc = {None: np.ones(D, bool), "num = 3": self.num == 3, "num = 1000": self.num == 1000, "num >= 0": self.num >= 0, "idx = %d" % (D - 1): self.idx == D - 1,
               "num >= 30 AND tag = 't1'": (self.num >= 30) & (self.tag == "t1"), "num < 20": self.num < 20, "tag = 't1'": self.tag == "t1", "tag = 't2'": self.tag == "t2",
               "tag = 't3'": self.tag == "t3"}
        return acc[x] & self.live

    @staticmethod
    def figures(v):
        """(count, nan, min, max, sum, mean) of the values v of one slot"""
        if v.dtype.kind != "f":
            ints = [int(x) for x in v]
            total = sum(ints)
            return len(ints), 0, min(ints) if ints else None, max(ints) if ints else None, total, float(Fraction(total, len(ints))) if ints else None
        nan = int(np.isnan(v).sum()); w = v[~np.isnan(v)]; fin = [float(x) for x in w[np.isfinite(w)]]
        pinf, ninf = int((w == np.inf).sum()), int((w == -np.inf).sum())
        if pinf or ninf:
            total = mean = float("nan") if pinf and ninf else (np.inf if pinf else -np.inf)
        else:
            total = math.fsum(fin)
            mean = float(sum((Fraction(x) for x in fin), Fraction(0)) / len(fin)) if fin else None
            assert total == float(sum((Fraction(x) for x in fin), Fraction(0)))
        return len(w), nan, float(w.min()) if len(w) else None, float(w.max()) if len(w) else None, float(total), None if not len(w) else float(mean)

    def stats(self, r):
        """(count, nan, total, min, max, sum, mean, [(value, count, nan, min, max, sum, mean)]) of a StatsRequest"""
        live = self.members(r.filter)
        col = getattr(self, r.field)
        count, nan, lo, up, total, mean = self.figures(col[live])
        groups = []
        if r.group_by is not None:
            g = getattr(self, r.group_by)
            for gv in np.unique(g[live]):
                groups.append((str(gv),) + self.figures(col[live & (g == gv)]))
            groups.sort(key=lambda x: (-(x[1] + x[2]), x[0]))          # members descending, then the value's text ascending (ASCII here)
        return count, nan, int(live.sum()), lo, up, total, mean, groups


def same(a, b):
    """== that also holds between two NaNs"""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def check(m, got, r):
    want = m.stats(r)
    assert got.error is None, (r, got.error)
    have = (got.count, got.nan, got.total, got.min, got.max, got.sum, got.mean)
    assert all(same(x, y) for x, y in zip(have, want[:7])), (r, have, want[:7])
    assert len(got.groups) == len(want[7]), (r, len(got.groups), len(want[7]))
    for g, w in zip(got.groups, want[7]):
        have = (g.value, g.count, g.nan, g.min, g.max, g.sum, g.mean)
        assert all(same(x, y) for x, y in zip(have, w)), (r, have, w)


def build(m):
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(int(k), "word%d item %d of the shelf" % (i % 11, i)) for i, k in enumerate(m.keys)])
    for name in ("idx", "num", "g1000", "g3000", "qty", "big", "price", "four", "infs", "wild"):
        e.set_column(name, getattr(m, name), facetable=name == "num")
    e.set_column("tag", list(m.tag), facetable=True); e.set_column("one", list(m.one))
    assert e.delete_documents(m.keys[~m.live]) == 3
    return e


@pytest.fixture(scope="module")
def fx():
    m = Model()
    return build(m), m


def test_the_columns_are_what_the_cases_need():
    m = Model()
    assert [limbs(getattr(m, f)) for f in ("qty", "big", "price", "four")] == [1, 2, 3, 4] and limbs(m.wild) > 4
    fin = m.price[np.isfinite(m.price)]
    exact = sum((Fraction(float(x)) for x in fin), Fraction(0))
    assert math.fsum(fin) == float(exact) and sum(int(x) for x in m.big) > 2 ** 64


def test_every_field_filter_and_grouping_equals_numpy(fx):
    e, m = fx
    reqs = [StatsRequest(f, field, g) for field in FIELDS for f in FILTERS for g in (None, "tag", "one")]
    got = e.field_stats(reqs)                                    # ninety requests: sixteen per device call
    assert len(got) == len(reqs) == 90
    for r, a in zip(reqs, got):
        check(m, a, r)
    assert e.last_field_stats_stats()[2] == 1
    whole = e.field_stats(None, "infs")
    assert math.isnan(whole.sum) and math.isnan(whole.mean) and whole.nan > 0
    by = {g.value: g for g in e.field_stats(None, "infs", "tag").groups}
    assert by["t1"].sum == np.inf and by["t2"].sum == -np.inf and math.isnan(by["t3"].sum) and by["t1"].max == np.inf and by["t2"].min == -np.inf
    assert isinstance(e.field_stats(None, "big").sum, int) and abs(e.field_stats(None, "big").sum) > 2 ** 64
    last = e.field_stats("idx = %d" % (D - 1), "price", "tag")   # only the corpus's partial last walk group
    assert (last.total, last.sum, last.mean, [g.value for g in last.groups]) == (1, 12.25, 12.25, ["t%d" % ((D - 1) % 7)])
    none = e.field_stats("num = 1000", "price", "tag")
    assert (none.count, none.nan, none.total, none.min, none.max, none.sum, none.mean, none.groups) == (0, 0, 0, None, None, 0.0, None, [])
    assert e.field_stats("num = 1000", "qty").sum == 0 and type(e.field_stats("num = 1000", "qty").sum) is int


def test_large_group_columns_in_lds_and_in_global_memory_agree(fx):
    """Slots x words against the placement rule: 1000 groups fit the 16 384 words of a 256-thread workgroup alone (8 000 words with one limb, 12 000 with
    three) and not all of them side by side; 3000 groups of one or three limbs (24 000 / 36 000 words) need the whole LDS of a CU, the 1024-thread launch;
    3000 groups of four limbs (42 000 words) fit nowhere and are added in global memory.  Inside the call of sixteen the small budget leaves several
    requests out, the large one fewer: one launch with slots in LDS and in global memory.  The same request gives the same answer wherever its slots lie."""
    e, m = fx
    for r in (StatsRequest(None, "price", "g3000"), StatsRequest("num < 20", "price", "g3000"), StatsRequest(None, "qty", "g3000"), StatsRequest(None, "price", "g1000"),
              StatsRequest(None, "qty", "g1000"), StatsRequest("num < 20", "four", "g1000"), StatsRequest(None, "four", "g3000"), StatsRequest("num < 20", "big", "g3000")):
        alone = e.field_stats(r.filter, r.field, r.group_by)
        check(m, alone, r)
        assert e.last_field_stats_stats()[2] == 1
        fill = [StatsRequest(f, field, g) for f in ("num < 20", None, "tag = 't1'") for field, g in (("qty", "g1000"), ("price", "tag"), ("four", None), ("big", "one"), ("price", "g1000"))]
        call = fill[:7] + [r] + fill[7:]
        assert len(call) == 16
        got = e.field_stats(call)
        assert e.last_field_stats_stats()[2] == 1                # ONE launch for the sixteen
        assert repr(got[7]) == repr(alone)
        for q, a in zip(call, got):
            check(m, a, q)


def test_a_field_grouped_by_itself(fx):
    e, m = fx
    r = StatsRequest("num < 20", "qty", "qty")
    got = e.field_stats(r.filter, r.field, r.group_by)
    check(m, got, r)
    assert all(g.min == g.max == int(g.value) and g.sum == g.count * int(g.value) for g in got.groups)
    assert sum(g.sum for g in got.groups) == got.sum and sum(g.count for g in got.groups) == got.count


def test_group_figures_add_up_to_the_whole(fx):
    e, m = fx
    for field in FIELDS:
        for g in ("tag", "g3000"):
            a = e.field_stats("num >= 0", field, g)
            assert sum(x.count for x in a.groups) == a.count and sum(x.nan for x in a.groups) == a.nan and a.count + a.nan == a.total == int(m.live.sum())
            if field in ("qty", "big"):
                assert sum(x.sum for x in a.groups) == a.sum
            counts = [x.count + x.nan for x in a.groups]
            assert counts == sorted(counts, reverse=True) and min(counts) >= 1


def test_sixteen_requests_are_one_launch_and_seventeen_two_calls(fx):
    e, m = fx
    s = Session(e)
    try:
        reqs = [StatsRequest("num = %d" % 3 if i % 2 else None, FIELDS[i % 5], (None, "tag", "one")[i % 3]) for i in range(17)]
        got = s.field_stats(reqs[:16])
        assert s.last_field_stats_stats() == (1, 0, 1)
        more = s.field_stats(reqs)
        assert s.last_field_stats_stats() == (0, 0, 1)           # the second call: request seventeen alone, no filter
        assert [repr(x) for x in more[:16]] == [repr(x) for x in got]
        for r, a in zip(reqs, more):
            check(m, a, r)
    finally:
        s.close()


def test_a_refused_request_beside_answered_ones(fx):
    e, m = fx
    reqs = [StatsRequest(None, "price", "tag"), StatsRequest(None, "wild"), StatsRequest(None, "nosuch"), StatsRequest("num = ", "qty"), StatsRequest("tag MATCHES 't[12]'", "qty"),
            StatsRequest(None, "tag"), StatsRequest(None, None), StatsRequest(None, "qty", "nosuch"), StatsRequest(None, "qty", "idx"), StatsRequest("num = 3", "big", "one")]
    got = e.field_stats(reqs)
    for i in (0, 9):
        check(m, got[i], reqs[i])
    for i in range(1, 9):
        assert got[i].error and (got[i].count, got[i].total, got[i].sum, got[i].groups) == (0, 0, 0, []), (i, got[i])
    assert "128 binary digits" in got[1].error and "nosuch" in got[2].error and "syntax" in got[3].error and "string" in got[5].error and "4096" in got[8].error
    one = e.field_stats(None, "wild")
    assert one.error and "128 binary digits" in one.error


def test_two_sessions_and_repeated_calls_return_the_same_bytes(fx):
    e, m = fx
    reqs = [StatsRequest(f, field, g) for f in (None, "num < 20") for field, g in (("price", None), ("price", "tag"), ("four", "g3000"), ("infs", "tag"), ("big", "g1000"))]
    a, b = Session(e), Session(e)
    try:
        first = repr(a.field_stats(reqs))
        for s in (a, b, a, b):
            assert repr(s.field_stats(reqs)) == first
        assert repr([s.field_stats(r.filter, r.field, r.group_by) for s, r in zip((a, b) * 5, reqs)]) == first      # one by one, another order of calls
    finally:
        a.close(); b.close()


def test_masks_are_shared_with_list_documents(fx):
    e, m = fx
    s = Session(e)
    try:
        s.list_documents("num < 20", "qty", True, 0, 10)
        assert s.last_list_stats()[:2] == (1, 0)
        r = StatsRequest("num < 20", "price", "tag")
        check(m, s.field_stats(r.filter, r.field, r.group_by), r)
        assert s.last_field_stats_stats() == (0, 1, 1)           # the listing's mask, reused
        r = StatsRequest("tag = 't2'", "qty")
        check(m, s.field_stats(r.filter, r.field), r)
        assert s.last_field_stats_stats() == (1, 0, 1)
        got = s.list_documents([ListRequest("tag = 't2'", None, True, 0, 5), ListRequest("num < 20", None, True, 0, 5)])
        assert s.last_list_stats()[:2] == (0, 2)                 # and the other way round
        assert got[0].total == int(m.members("tag = 't2'").sum()) == s.field_stats("tag = 't2'", "qty").total
    finally:
        s.close()


def test_a_deletion_changes_the_answers():
    m = Model()
    e = build(m)
    r = StatsRequest("num < 20", "price", "tag")
    before = e.field_stats(r.filter, r.field, r.group_by)
    check(m, before, r)
    gone = np.nonzero(m.members("num < 20"))[0][:9]
    assert e.delete_documents(m.keys[gone]) == 9
    m.live[gone] = False
    after = e.field_stats(r.filter, r.field, r.group_by)
    check(m, after, r)
    assert after.total == before.total - 9 and e.last_field_stats_stats()[:2] == (1, 0)      # the mask was built again
    for q in (StatsRequest(None, "big", "g3000"), StatsRequest(None, "qty")):
        check(m, e.field_stats(q.filter, q.field, q.group_by), q)
    e.restore_documents()
    m.live[:] = True
    check(m, e.field_stats(r.filter, r.field, r.group_by), r)


def test_a_replaced_column_is_answered_from_its_new_values():
    m = Model()
    e = build(m)
    r = StatsRequest("num < 20", "price", "tag")
    check(m, e.field_stats(r.filter, r.field, r.group_by), r)
    rng = np.random.default_rng(3)
    m.price = rng.integers(-1000, 1000, D) * 2.0 ** 200 + rng.integers(0, 2, D) * 2.0 ** 150      # another scale, two limbs
    assert limbs(m.price) == 2
    e.set_column("price", m.price)
    for q in (r, StatsRequest(None, "price"), StatsRequest(None, "price", "g3000"), StatsRequest(None, "qty", "tag")):
        check(m, e.field_stats(q.filter, q.field, q.group_by), q)
    m.price = np.where(np.arange(D) % 2 == 0, 1e-30, 1e30)      # and by values that cannot be summed exactly: refused; the other columns still answer
    e.set_column("price", m.price)
    assert "128 binary digits" in e.field_stats(None, "price").error
    check(m, e.field_stats(None, "qty", "tag"), StatsRequest(None, "qty", "tag"))
