"""bucket_stats on the GPU: field_stats' figures — counts, NaNs, min / max and the EXACT sum and mean — of a numeric field over the members of every range
bucket of a second numeric field, over the documents a filter accepts.

Expected rows come from numpy on the columns' VALUES: membership in the set by numpy comparisons, membership in a row by comparing the bucket column's values
with the edges, the figures of a row by the model of tests/test_gpu_field_stats.py, restated here (an int column's sum as a Python int, a double column's by
math.fsum, the mean as float(Fraction(exact sum) / count)).  Every comparison is ==.
4 099 documents: 256 walk groups of 16 and a partial last one of three; three of them deleted.  Value columns: qty (small int64), big (int64 with both
extremes: a row's sum exceeds 64 bits), price (doubles of three limbs with NaNs, +-0.0, 2^-20 and values near +-1e11), four (doubles of four limbs), infs (both
infinities and NaNs), wild (1e-30 and 1e30: refused).  Bucket columns: idx (the document's number: buckets are runs of consecutive documents), num (random
ints 0 .. 99) and when (doubles with NaNs, both infinities and +-0.0)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from infidex_amd import BucketStatsRequest, Document, RangeRequest, SearchEngine, StatsRequest
from infidex_amd.engine import Session

pytestmark = pytest.mark.gpu

D = 4099
I64 = np.iinfo(np.int64)
INF = float("inf")
FILTERS = [None, "num = 3", "num = 1000", "num >= 0", "idx = %d" % (D - 1), "num >= 30 AND tag = 't1'"]
FIELDS = ["qty", "big", "price", "four", "infs"]
IDX1, IDX8, IDX256 = (0, D), tuple(range(0, 4097, 512)), tuple(range(3, 3 + 257 * 16, 16))      # 1, 8 and 256 buckets over idx; IDX256 leaves 3 below and none above
WHEN = (-INF, -10.0, -0.5, 0.0, 0.5, 10.0, INF)


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
        rng.permutation(D); rng.permutation(D)                     # (that file's two large group columns: drawn, so that the value columns below are the same)
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
        self.when = np.round(rng.normal(0.0, 8.0, D), 1)
        pick = rng.choice(D - 1, 90, replace=False)
        self.when[pick[:50]] = np.nan; self.when[pick[50:60]] = np.inf; self.when[pick[60:70]] = -np.inf; self.when[pick[70:80]] = -0.0; self.when[pick[80:]] = 0.0
        self.live = np.ones(D, bool); self.live[[0, 2048, D - 2]] = False
        self.memo = {}

    def members(self, x):
        """bool per document: live and accepted by filter x (the comparisons the tests use)"""
        acc = {None: np.ones(D, bool), "num = 3": self.num == 3, "num = 1000": self.num == 1000, "num >= 0": self.num >= 0, "idx = %d" % (D - 1): self.idx == D - 1,
               "num >= 30 AND tag = 't1'": (self.num >= 30) & (self.tag == "t1"), "num < 20": self.num < 20, "tag = 't1'": self.tag == "t1", "tag = 't2'": self.tag == "t2"}
        return acc[x] & self.live

    @staticmethod
    def figures(v):
        """(count, nan, min, max, sum, mean) of the values v of one row"""
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

    def row(self, col, mask):
        return (int(mask.sum()),) + self.figures(col[mask])

    def stats(self, r):
        """(rows in the order [below | buckets | above | nan], whole, total) of a BucketStatsRequest, each row (size, count, nan, min, max, sum, mean)"""
        key = (r.filter, r.field, r.bucket_by, tuple(r.edges))      # (a test that changes the model clears the memo)
        if key not in self.memo:
            live = self.members(r.filter)
            v, c, e = getattr(self, r.field), getattr(self, r.bucket_by), r.edges
            with np.errstate(invalid="ignore"):
                masks = [c < e[0]] + [(c >= e[i]) & (c < e[i + 1]) for i in range(len(e) - 1)] + [c >= e[-1]] + [np.isnan(c) if c.dtype.kind == "f" else np.zeros(D, bool)]
            self.memo[key] = ([self.row(v, live & m) for m in masks], self.row(v, live), int(live.sum()))
        return self.memo[key]


def same(a, b):
    """== that also holds between two NaNs"""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def flat(row):
    return (row.size, row.count, row.nan, row.min, row.max, row.sum, row.mean)


def check(m, got, r):
    rows, whole, total = m.stats(r)
    assert got.error is None, (r, got.error)
    assert got.edges == tuple(r.edges) and len(got.buckets) == len(r.edges) - 1 and got.total == total
    have = [got.below] + got.buckets + [got.above, got.nan]
    for k, (g, w) in enumerate(zip(have, rows)):
        assert all(same(x, y) for x, y in zip(flat(g), w)), (r.filter, r.field, r.bucket_by, k, flat(g), w)
        assert g.size == g.count + g.nan
    assert all(same(x, y) for x, y in zip(flat(got.whole), whole)), (r, flat(got.whole), whole)
    # the invariants of the contract
    assert got.nan.size + got.below.size + sum(b.size for b in got.buckets) + got.above.size == got.total == got.whole.size
    assert sum(x.count for x in have) == got.whole.count and sum(x.nan for x in have) == got.whole.nan
    if isinstance(got.whole.sum, int):
        assert sum(x.sum for x in have) == got.whole.sum


def build(m):
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(int(k), "word%d item %d of the shelf" % (i % 11, i)) for i, k in enumerate(m.keys)])
    for name in ("idx", "num", "qty", "big", "price", "four", "infs", "wild", "when"):
        e.set_column(name, getattr(m, name), facetable=name == "num")
    e.set_column("tag", list(m.tag), facetable=True)
    assert e.delete_documents(m.keys[~m.live]) == 3
    return e


@pytest.fixture(scope="module")
def fx():
    m = Model()
    return build(m), m


def test_the_columns_are_what_the_cases_need():
    m = Model()
    assert [limbs(getattr(m, f)) for f in ("qty", "big", "price", "four")] == [1, 2, 3, 4] and limbs(m.wild) > 4
    assert np.isnan(m.when).sum() == 50 and np.isinf(m.when).sum() == 20 and len(IDX8) == 9 and len(IDX256) == 257 and IDX256[-1] >= D
    assert abs(sum(int(x) for x in m.big[m.live])) > 2 ** 64


def test_every_field_filter_and_bucketing_equals_numpy(fx):
    e, m = fx
    B = BucketStatsRequest
    reqs = [B(f, field, by, edges) for field in FIELDS for f in FILTERS for by, edges in (("idx", IDX1), ("idx", IDX8), ("when", WHEN))]
    got = e.bucket_stats(reqs)                                    # ninety requests: sixteen per device call
    assert len(got) == len(reqs) == 90
    for r, a in zip(reqs, got):
        check(m, a, r)
    assert e.last_bucket_stats_stats()[2] == 1
    # the sizes are range_facets' counters and the whole is field_stats', for the same filters and edges
    facets = e.range_facets([RangeRequest(r.filter, r.bucket_by, r.edges) for r in reqs])
    stats = e.field_stats([StatsRequest(r.filter, r.field) for r in reqs])
    for r, a, f, s in zip(reqs, got, facets, stats):
        assert ([x.size for x in a.buckets], a.below.size, a.above.size, a.nan.size, a.total) == (f.counts, f.below, f.above, f.nan, f.total), r
        assert repr((a.whole.count, a.whole.nan, a.whole.min, a.whole.max, a.whole.sum, a.whole.mean)) == repr((s.count, s.nan, s.min, s.max, s.sum, s.mean)) and a.total == s.total, r
    one = e.bucket_stats(None, "infs", "idx", IDX1)               # both infinities in one row: the sum and the mean are NaNs
    assert math.isnan(one.buckets[0].sum) and math.isnan(one.buckets[0].mean) and one.buckets[0].nan > 0 and one.buckets[0].min == -INF and one.buckets[0].max == INF
    big = e.bucket_stats(None, "big", "idx", IDX1).buckets[0]     # a row's sum beyond 64 bits
    assert type(big.sum) is int and abs(big.sum) > 2 ** 64
    nan = e.bucket_stats(None, "qty", "when", WHEN)               # NaN in bucket_by: the nan row; -inf and +inf values lie in the first bucket and above
    assert nan.nan.size == int((np.isnan(m.when) & m.live).sum()) > 0 and nan.below.size == 0 and nan.above.size == int(((m.when == INF) & m.live).sum()) > 0
    last = e.bucket_stats("idx = %d" % (D - 1), "price", "idx", IDX8)      # only the corpus's partial last walk group
    assert (last.total, last.above.size, last.above.sum, last.above.mean, last.whole.sum) == (1, 1, 12.25, 12.25, 12.25) and all(b.size == 0 for b in last.buckets)
    none = e.bucket_stats("num = 1000", "price", "idx", IDX8)    # the empty set: every row reads as field_stats on an empty set
    assert none.total == 0 and all(flat(x) == (0, 0, 0, None, None, 0.0, None) for x in none.buckets + [none.below, none.above, none.nan, none.whole])
    none = e.bucket_stats("num = 1000", "qty", "idx", IDX8)
    assert all(flat(x) == (0, 0, 0, None, None, 0, None) and type(x.sum) is int for x in none.buckets + [none.below, none.above, none.nan, none.whole])


def test_everything_below_everything_above_and_empty_buckets_between(fx):
    e, m = fx
    B = BucketStatsRequest
    reqs = [B("num >= 0", "price", "idx", (D + 10, D + 20)), B("num >= 0", "qty", "idx", (-20, -10)), B(None, "four", "idx", (0, 100, 5000, 6000, 7000)),
            B("num < 20", "big", "num", (-5, 0, 50, 200, 300)), B(None, "price", "when", (-INF, -1e300, 1e300, INF)), B(None, "infs", "when", (100.0, 200.0)),
            B("tag = 't1'", "qty", "num", tuple(range(-78, 179)))]                    # 256 buckets of width one, most of them empty
    got = e.bucket_stats(reqs)
    for r, a in zip(reqs, got):
        check(m, a, r)
    total = int(m.live.sum())
    assert got[0].below.size == total and got[0].above.size == 0 and got[1].above.size == total and got[1].below.size == 0
    assert [b.size for b in got[2].buckets[2:]] == [0, 0] and got[2].above.size == 0 and [b.size for b in got[3].buckets[2:]] == [0, 0]
    assert sum(1 for b in got[6].buckets if b.size == 0) >= 156


def test_a_field_bucketed_by_itself(fx):
    e, m = fx
    B = BucketStatsRequest
    reqs = [B("num < 20", "qty", "qty", (-5, 0, 10, 40)), B(None, "price", "price", (-1e12, 0.0, 50.0, 1e12)), B("num >= 0", "idx", "idx", IDX256), B(None, "infs", "infs", (-INF, 0.0, INF))]
    got = e.bucket_stats(reqs)
    for r, a in zip(reqs, got):
        check(m, a, r)
    assert all(b.min >= lo and b.max < up for b, lo, up in zip(got[0].buckets, (-5, 0, 10), (0, 10, 40)))
    assert got[1].nan.size == got[1].nan.nan == int((np.isnan(m.price) & m.live).sum()) >= 37 and got[1].nan.count == 0 and got[1].nan.sum == 0.0 and got[1].nan.mean is None      # NaN in bucket_by and in field at once
    assert all(b.size in (15, 16) and b.sum == sum(range(b.min, b.max + 1)) - sum(x for x in (2048,) if b.min <= x <= b.max) for b in got[2].buckets[:255])
    assert got[3].above.sum == INF and got[3].buckets[0].sum == -INF and got[3].buckets[0].min == -INF


def test_every_row_is_field_stats_of_the_composed_filter(fx):
    """For an int bucket column a row's members are a filter of their own: row == field_stats("F AND c >= e_i AND c < e_(i+1)", v).  Six composed filters and F
    itself: seven masks of the session's sixteen."""
    e, m = fx
    edges = (10, 20, 35, 50, 90)
    s = Session(e)
    try:
        for F in (None, "tag = 't1'"):
            pre = "" if F is None else F + " AND "
            exprs = [pre + "num < 10"] + [pre + "num >= %d AND num < %d" % (a, b) for a, b in zip(edges, edges[1:])] + [pre + "num >= 90"]
            for field in ("price", "big", "four", "infs"):
                a = s.bucket_stats(F, field, "num", edges)
                assert a.error is None
                want = s.field_stats([StatsRequest(x, field) for x in exprs])
                for row, w in zip([a.below] + a.buckets + [a.above], want):
                    assert w.error is None and repr(flat(row)) == repr((w.total, w.count, w.nan, w.min, w.max, w.sum, w.mean)), (F, field)
                assert a.nan.size == 0
    finally:
        s.close()


def test_slots_in_small_lds_big_lds_and_global_memory_agree(fx):
    """Slots x words against the placement rule.  A request of 256 buckets over a four-limb field is 259 x 14 = 3 626 words: alone it lies in a workgroup's LDS;
    sixteen of them are 58 016 words and do not fit the whole LDS of a CU (40 960 words less the thresholds): one launch of 1024 threads with the slots of some
    requests in LDS and of the others in global memory.  The same request gives the same bytes wherever its slots lie, on either session."""
    e, m = fx
    B = BucketStatsRequest
    r = B("num < 20", "four", "idx", IDX256)
    a, b = Session(e), Session(e)
    try:
        alone = a.bucket_stats(r.filter, r.field, r.bucket_by, r.edges)
        check(m, alone, r)
        assert a.last_bucket_stats_stats()[2] == 1 and a.last_bucket_stats_placement() == (1, 0, 0)
        wide = tuple(range(-78, 179))
        fill = [B(f, "four", by, edges) for f in ("num < 20", None, "tag = 't1'") for by, edges in (("idx", IDX256), ("num", wide), ("idx", tuple(x + 1 for x in IDX256)))]
        fill += [B(f, "four", "when", tuple(float(x) / 8 for x in range(-128, 129))) for f in ("num < 20", None, "tag = 't1'")]
        call = fill[1:8] + [r] + fill[8:12] + fill[:1] + fill[1:4]
        assert len(call) == 16 and all(len(q.edges) == 257 and q.field == "four" for q in call)
        got = a.bucket_stats(call)
        small, big, glob = a.last_bucket_stats_placement()
        assert a.last_bucket_stats_stats()[2] == 1 and small == 0 and big >= 1 and glob >= 1 and big + glob == 16, (small, big, glob)      # ONE launch, and the global path ran
        assert repr(got[7]) == repr(alone) and repr(got[12]) == repr(alone) and repr(got[13]) == repr(got[0])
        for q, x in zip(call, got):
            check(m, x, q)
        # the same sixteen without the big launch shape would be the small one: a call whose slots fit the small budget instead
        few = [B("num < 20", "qty", "idx", IDX8), r, B(None, "price", "when", WHEN), B("num < 20", "big", "num", (0, 50, 100))]
        got4 = b.bucket_stats(few)
        assert b.last_bucket_stats_placement() == (4, 0, 0) and b.last_bucket_stats_stats() == (1, 0, 1)
        assert repr(got4[1]) == repr(alone)
        for q, x in zip(few, got4):
            check(m, x, q)
        assert repr(b.bucket_stats(call)) == repr(got) and repr(a.bucket_stats(few)) == repr(got4)      # the other session: the same bytes
        # more slots than a workgroup's budget and fewer than a CU's: the 1024-thread launch with every request in LDS
        mid = call[:8]
        got8 = a.bucket_stats(mid)
        assert a.last_bucket_stats_placement() == (0, 8, 0) and repr(got8) == repr(got[:8])
    finally:
        a.close(); b.close()


def test_sixteen_requests_are_one_launch_and_seventeen_two_calls(fx):
    e, m = fx
    s = Session(e)
    try:
        reqs = [BucketStatsRequest("num = 3" if i % 2 else None, FIELDS[i % 5], ("idx", "when", "num")[i % 3], (IDX8, WHEN, (0, 25, 50, 75, 100))[i % 3]) for i in range(17)]
        got = s.bucket_stats(reqs[:16])
        assert s.last_bucket_stats_stats() == (1, 0, 1)
        more = s.bucket_stats(reqs)
        assert s.last_bucket_stats_stats() == (0, 0, 1) and s.last_bucket_stats_placement() == (1, 0, 0)      # the second call: request seventeen alone, no filter
        assert [repr(x) for x in more[:16]] == [repr(x) for x in got]
        for r, a in zip(reqs, more):
            check(m, a, r)
    finally:
        s.close()


def test_a_refused_request_beside_answered_ones(fx):
    e, m = fx
    B = BucketStatsRequest
    reqs = [B(None, "price", "idx", IDX8), B(None, "wild", "idx", IDX8), B(None, "nosuch", "idx", IDX8), B("num = ", "qty", "idx", IDX8), B("tag MATCHES 't[12]'", "qty", "idx", IDX8),
            B(None, "tag", "idx", IDX8), B(None, None, "idx", IDX8), B(None, "qty", "nosuch", IDX8), B(None, "qty", "tag", IDX8), B(None, "qty", None, IDX8),
            B(None, "qty", "idx", (5, 5)), B(None, "qty", "idx", (5,)), B(None, "qty", "idx", (0.5, 1.5)), B(None, "qty", "when", (0.0, float("nan"))),
            B(None, "qty", "when", (-0.0, 0.0)), B("num = 3", "big", "when", WHEN)]
    got = e.bucket_stats(reqs)
    for i in (0, 15):
        check(m, got[i], reqs[i])
    for i in range(1, 15):
        assert got[i].error and (got[i].edges, got[i].buckets, got[i].total, got[i].whole) == (tuple(reqs[i].edges), [], 0, BucketStats_row()), (i, got[i])
    words = {1: "128 binary digits", 2: "no field named 'nosuch'", 3: "syntax", 5: "field 'tag' is a string column", 6: "needs a field", 7: "no bucket_by field named 'nosuch'",
             8: "bucket_by field 'tag' is a string column", 9: "needs a bucket_by field", 10: "strictly increasing", 11: "2 to 257 edges", 12: "integer column needs integer edges",
             13: "not a NaN", 14: "strictly increasing"}
    for i, w in words.items():
        assert w in got[i].error and (i in (3,) or got[i].error.startswith("bucket_stats")), (i, got[i].error)
    one = e.bucket_stats(None, "wild", "idx", IDX8)
    assert one.error and "128 binary digits" in one.error


def BucketStats_row():
    from infidex_amd import BucketRow
    return BucketRow()


def test_masks_are_shared_with_field_stats_and_only_masks_are_cached(fx):
    e, m = fx
    s = Session(e)
    try:
        s.field_stats("num < 20", "qty")
        r = BucketStatsRequest("num < 20", "price", "when", WHEN)
        check(m, s.bucket_stats(r.filter, r.field, r.bucket_by, r.edges), r)
        assert s.last_bucket_stats_stats() == (0, 1, 1)           # field_stats' mask, reused; the pass itself runs again
        check(m, s.bucket_stats(r.filter, r.field, r.bucket_by, r.edges), r)
        assert s.last_bucket_stats_stats() == (0, 1, 1)
    finally:
        s.close()


def test_deletions_a_restore_and_a_replaced_bucket_column_change_the_answers():
    m = Model()
    e = build(m)
    r = BucketStatsRequest("num < 20", "price", "num", (0, 5, 10, 15, 20))
    q = BucketStatsRequest(None, "big", "when", WHEN)
    before = e.bucket_stats(r.filter, r.field, r.bucket_by, r.edges)
    check(m, before, r); check(m, e.bucket_stats(q.filter, q.field, q.bucket_by, q.edges), q)
    gone = np.nonzero(m.members("num < 20"))[0][:9]
    assert e.delete_documents(m.keys[gone]) == 9
    m.live[gone] = False; m.memo.clear()
    after = e.bucket_stats(r.filter, r.field, r.bucket_by, r.edges)
    check(m, after, r); check(m, e.bucket_stats(q.filter, q.field, q.bucket_by, q.edges), q)
    assert after.total == before.total - 9 and e.last_bucket_stats_stats()[:2] == (0, 0)      # (q has no filter; r's mask was built again just before)
    e.restore_documents()
    m.live[:] = True; m.memo.clear()
    check(m, e.bucket_stats(r.filter, r.field, r.bucket_by, r.edges), r)
    # bucket_by replaced: other values, another dictionary, another sort rank; the filter "num < 20" reads the new values too
    m.when = np.where(np.arange(D) % 3 == 0, np.nan, (np.arange(D) % 41 - 20) / 4.0)
    e.set_column("when", m.when); m.memo.clear()
    got = e.bucket_stats(q.filter, q.field, q.bucket_by, q.edges)
    check(m, got, q)
    assert got.nan.size == int(np.isnan(m.when).sum()) and got.above.size == 0
    m.num = (np.arange(D, dtype=np.int64) * 7) % 23
    e.set_column("num", m.num, facetable=True); m.memo.clear()
    check(m, e.bucket_stats(r.filter, r.field, r.bucket_by, r.edges), r)
