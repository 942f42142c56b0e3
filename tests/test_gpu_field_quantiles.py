"""field_quantiles on the GPU: the value at position floor((count - 1) * q) of a numeric field over the documents a filter accepts, whole and per group.

Expected values come from numpy on the columns' VALUES: membership by numpy comparisons, np.sort(v[~isnan])[floor((c - 1) * q)], and
numpy.quantile(method="lower") as a second opinion where numpy computes it without rounding.  Every comparison is ==.
4 099 documents: 256 walk groups of 16 and a partial last one of three; three of them deleted, one in the last group.  Value columns: qty (small int64,
heavy ties), big (int64 with both extremes), price (doubles with NaNs, +-0.0, +-inf and repeated values), uniq (all distinct).  Group columns: tag (7
strings), one (a single value), g1000 and g3000 (ints: by size their bins lie in a workgroup's LDS, in a CU's whole LDS or in global memory), qty by
itself.  A second corpus of 70 001 documents carries a column of 70 001 values: 17 bits of keys, two passes at 11-bit digits and five at 4."""
import math

import numpy as np
import pytest

from infidex_amd import Document, ListRequest, QuantileRequest, SearchEngine
from infidex_amd import engine as E
from infidex_amd.engine import Session

pytestmark = pytest.mark.gpu

D = 4099
I64 = np.iinfo(np.int64)
FILTERS = [None, "num = 3", "num = 1000", "idx = %d" % (D - 1), "num >= 30 AND tag = 't1'"]
FIELDS = ["qty", "big", "price", "uniq"]
Q_MEDIAN, Q_ENDS, Q_BOX = (0.5,), (0, 1), (0, 0.25, 0.5, 0.75, 1)
Q_SIXTEEN = (0.9, 0.1, 0.5, 0.5, 1 / 3, 0.999, 0.0, 1.0, 0.75, 0.25, 0.1, 0.95, 0.05, 0.5, 1.0, 0.01)
QSETS = [Q_MEDIAN, Q_ENDS, Q_BOX, Q_SIXTEEN]


class Model:
    def __init__(self, d=D, seed=11):
        rng = np.random.default_rng(seed)
        self.d = d
        self.keys = np.arange(d, dtype=np.int64) * 3 + 1000
        self.idx = np.arange(d, dtype=np.int64)
        self.num = rng.integers(0, 100, d).astype(np.int64)
        self.tag = np.array(["t%d" % (i % 7) for i in range(d)])
        self.one = np.array(["only"] * d)
        self.g1000 = (rng.permutation(d) % 1000).astype(np.int64)
        self.g3000 = (rng.permutation(d) % 3000).astype(np.int64)
        self.qty = rng.integers(-5, 40, d).astype(np.int64)
        self.big = rng.integers(-2 ** 62, 2 ** 62, d).astype(np.int64)
        self.big[rng.choice(d, min(d, 200), replace=False)] = I64.max; self.big[rng.choice(d, min(d, 90), replace=False)] = I64.min; self.big[d - 1] = I64.max
        self.price = np.round(rng.normal(50.0, 30.0, d), 0)              # whole numbers: many repeated values
        pick = rng.choice(d - 1, min(d - 1, 400), replace=False)
        self.price[pick[:250]] = np.nan; self.price[pick[250:300]] = np.inf; self.price[pick[300:360]] = -np.inf
        self.price[pick[360:380]] = -0.0; self.price[pick[380:]] = 0.0; self.price[d - 1] = 12.25
        self.uniq = rng.permutation(d).astype(np.int64) * 7 - 9000
        self.live = np.ones(d, bool)
        if d == D:
            self.live[[0, 2048, d - 2]] = False

    def members(self, x):
        """bool per document: live and accepted by filter x (the comparisons the tests use)"""
        acc = {None: np.ones(self.d, bool), "num = 3": self.num == 3, "num = 1000": self.num == 1000, "idx = %d" % (self.d - 1): self.idx == self.d - 1,
               "num >= 30 AND tag = 't1'": (self.num >= 30) & (self.tag == "t1"), "num < 20": self.num < 20, "tag = 't2'": self.tag == "t2"}
        return acc[x] & self.live

    @staticmethod
    def figures(v, q):
        """(count, nan, values) of the values v of one slot"""
        isf = v.dtype.kind == "f"
        nan = int(np.isnan(v).sum()) if isf else 0
        w = np.sort(v[~np.isnan(v)] if isf else v)
        c = len(w)
        if not c:
            return 0, nan, [None] * len(q)
        vals = [w[math.floor((c - 1) * float(x))] for x in q]
        if (isf and np.isfinite(w).all()) or (not isf and np.abs(w.astype(np.float64)).max() < 2.0 ** 52):      # (numpy's own pick, where it takes no detour through arithmetic that rounds)
            assert [float(x) for x in np.quantile(w, [float(x) for x in q], method="lower")] == [float(x) for x in vals]
        return c, nan, [float(x) if isf else int(x) for x in vals]

    def quantiles(self, r):
        """(q, values, count, nan, total, [(value, count, nan, values)]) of a QuantileRequest"""
        live = self.members(r.filter)
        col = getattr(self, r.field)
        q = tuple(float(x) for x in r.q)
        count, nan, vals = self.figures(col[live], q)
        groups = []
        if r.group_by is not None:
            g = getattr(self, r.group_by)
            for gv in np.unique(g[live]):
                groups.append((str(gv),) + self.figures(col[live & (g == gv)], q))
            groups.sort(key=lambda x: (-(x[1] + x[2]), x[0]))          # members descending, then the value's text ascending (ASCII here)
        return q, vals, count, nan, int(live.sum()), groups


def same(a, b):
    """== between values of one type (an int column answers ints, a double column floats; -0.0 and 0.0 share a sort rank)"""
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def check(m, got, r):
    want = m.quantiles(r)
    assert got.error is None, (r, got.error)
    have = (got.q, got.values, got.count, got.nan, got.total)
    assert all(same(x, y) for x, y in zip(have, want[:5])), (r, have, want[:5])
    assert got.count + got.nan == got.total
    assert len(got.groups) == len(want[5]), (r, len(got.groups), len(want[5]))
    for g, w in zip(got.groups, want[5]):
        have = (g.value, g.count, g.nan, g.values)
        assert all(same(x, y) for x, y in zip(have, w)), (r, have, w)


def build(m, names=("idx", "num", "g1000", "g3000", "qty", "big", "price", "uniq")):
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(int(k), "word%d item %d of the shelf" % (i % 11, i)) for i, k in enumerate(m.keys)])
    for name in names:
        e.set_column(name, getattr(m, name), facetable=name == "num")
    e.set_column("tag", list(m.tag), facetable=True); e.set_column("one", list(m.one))
    gone = m.keys[~m.live]
    assert e.delete_documents(gone) == len(gone)
    return e


@pytest.fixture(scope="module")
def fx():
    m = Model()
    return build(m), m


def test_the_columns_are_what_the_cases_need():
    m = Model()
    assert len(np.unique(m.uniq)) == D and len(np.unique(m.qty)) == 45 and m.big.min() == I64.min and m.big.max() == I64.max
    p = m.price
    assert np.isnan(p).sum() == 250 and (p == np.inf).sum() == 50 and (p == -np.inf).sum() == 60 and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
    assert len(np.unique(p[np.isfinite(p)])) < 300 and not m.live[D - 2] and D % 16 == 3
    assert m.members("num = 1000").sum() == 0 and m.members("idx = %d" % (D - 1)).sum() == 1


def test_every_field_filter_grouping_and_q_set_equals_numpy(fx):
    e, m = fx
    reqs = [QuantileRequest(f, field, QSETS[(i + j + k) % 4], g) for i, field in enumerate(FIELDS) for j, f in enumerate(FILTERS) for k, g in enumerate((None, "tag", "one"))]
    reqs += [QuantileRequest(None, field, q, g) for field in FIELDS for q in QSETS for g in (None, "tag")]
    got = e.field_quantiles(reqs)                                # ninety-two requests: sixteen per device call
    assert len(got) == len(reqs) == 92
    for r, a in zip(reqs, got):
        check(m, a, r)
    none = e.field_quantiles("num = 1000", "price", Q_BOX, "tag")
    assert (none.q, none.values, none.count, none.nan, none.total, none.groups) == (tuple(float(x) for x in Q_BOX), [None] * 5, 0, 0, 0, [])
    last = e.field_quantiles("idx = %d" % (D - 1), "price", Q_SIXTEEN, "tag")      # only the corpus's partial last walk group: one member answers every q
    assert (last.values, last.count, last.total, [(g.value, g.values) for g in last.groups]) == ([12.25] * 16, 1, 1, [("t%d" % ((D - 1) % 7), [12.25] * 16)])
    whole = e.field_quantiles(None, "price", Q_ENDS)
    assert whole.values == [-np.inf, np.inf] and whole.nan == int(np.isnan(m.price[m.live]).sum()) > 0
    assert e.field_quantiles(None, "big", (0.0, 1.0)).values == [int(I64.min), int(I64.max)]
    assert e.field_quantiles(None, "qty", 0.5).q == (0.5,)        # a number alone is one quantile


def test_q_0_and_1_are_field_stats_min_and_max(fx):
    e, m = fx
    for field in FIELDS:
        for f in FILTERS:
            for g in (None, "tag"):
                a = e.field_quantiles(f, field, Q_ENDS, g)
                s = e.field_stats(f, field, g)
                assert (a.count, a.nan, a.total) == (s.count, s.nan, s.total) and same(a.values, [s.min, s.max]), (field, f, g, a, s)
                assert [(x.value, x.count, x.nan) for x in a.groups] == [(x.value, x.count, x.nan) for x in s.groups]
                assert all(same(x.values, [y.min, y.max]) for x, y in zip(a.groups, s.groups))
                assert repr(a.values) == repr([s.min, s.max])     # byte for byte: the same code of a rank that -0.0 and 0.0 share


def test_every_answer_is_what_list_documents_lists_at_its_position(fx):
    e, m = fx
    row = {int(k): i for i, k in enumerate(m.keys)}
    for field in FIELDS:
        for f in (None, "num >= 30 AND tag = 't1'", "num = 3"):
            a = e.field_quantiles(f, field, Q_SIXTEEN)
            pos = [math.floor((a.count - 1) * q) for q in a.q]
            pages = e.list_documents([ListRequest(f, field, True, a.nan + p, 1) for p in pos])
            col = getattr(m, field)
            for v, page in zip(a.values, pages):
                assert page.total == a.total and len(page.document_ids) == 1 and col[row[page.document_ids[0]]] == v, (field, f, v, page)
            if a.nan:                                             # NaNs hold the lowest ranks: the row before the first answer's is one
                before = e.list_documents(f, field, True, a.nan - 1, 1)
                assert math.isnan(col[row[before.document_ids[0]]])


def test_large_group_columns_wherever_their_bins_lie(fx):
    """1000 and 3000 groups: pass 0 takes (2^w + 1) words per slot, a later pass q x 2^w — in a workgroup's 16 384 words of LDS, in the 40 960 of a CU or in
    global memory, by the rule field_stats places its slots with.  The same request gives the same answer alone and inside a call of sixteen, and the groups'
    counts add up to the whole's."""
    e, m = fx
    for r in (QuantileRequest(None, "qty", Q_BOX, "g1000"), QuantileRequest(None, "uniq", Q_BOX, "g3000"), QuantileRequest("num < 20", "price", Q_SIXTEEN, "g3000"),
              QuantileRequest(None, "big", Q_MEDIAN, "g1000"), QuantileRequest(None, "qty", Q_SIXTEEN, "qty")):
        alone = e.field_quantiles(r.filter, r.field, r.q, r.group_by)
        check(m, alone, r)
        assert sum(g.count for g in alone.groups) == alone.count and sum(g.nan for g in alone.groups) == alone.nan
        counts = [g.count + g.nan for g in alone.groups]
        assert counts == sorted(counts, reverse=True) and min(counts) >= 1
        fill = [QuantileRequest(f, field, q, g) for f in ("num < 20", None, "tag = 't2'")
                for field, q, g in (("qty", Q_BOX, "g1000"), ("price", Q_ENDS, "tag"), ("uniq", Q_SIXTEEN, None), ("big", Q_MEDIAN, "one"), ("price", Q_BOX, "g1000"))]
        call = fill[:7] + [r] + fill[7:]
        assert len(call) == 16
        got = e.field_quantiles(call)
        assert repr(got[7]) == repr(alone)
        for q, a in zip(call, got):
            check(m, a, q)
    by = e.field_quantiles("num < 20", "qty", Q_ENDS, "qty")      # a field grouped by itself: every quantile of a group is the group
    assert all(g.values == [int(g.value)] * 2 for g in by.groups)


def test_sixteen_mixed_requests_are_one_launch_per_pass_and_thirty_three_are_split(fx):
    e, m = fx
    s = Session(e)
    try:
        filters = (None, "num < 20", "tag = 't2'", "num >= 30 AND tag = 't1'")
        reqs = [QuantileRequest(filters[i % 4], FIELDS[i % 4], QSETS[(i // 4) % 4], (None, "tag", "one", "g1000")[(i // 2) % 4]) for i in range(16)]
        alone = [s.field_quantiles(r.filter, r.field, r.q, r.group_by) for r in reqs]
        got = s.field_quantiles(reqs)
        built, reused, passes, launches = s.last_field_quantiles_stats()
        # uniq's 4 099 values are 13 bits of keys: two passes at 11-bit digits, each ONE k_quant_hist and one k_quant_pick launch for all sixteen
        assert (built, reused, passes, launches) == (0, 3, 2, 4)
        assert [repr(x) for x in got] == [repr(x) for x in alone]
        for r, a in zip(reqs, got):
            check(m, a, r)
        more = s.field_quantiles(reqs + reqs + reqs[:1])           # 33 requests: three device calls, the last of one request without a filter
        assert len(more) == 33 and [repr(x) for x in more] == [repr(x) for x in got + got + got[:1]]
        assert s.last_field_quantiles_stats() == (0, 0, 1, 2)     # qty alone: 45 values, one pass
    finally:
        s.close()


def test_a_refused_request_beside_answered_ones(fx):
    e, m = fx
    reqs = [QuantileRequest(None, "price", Q_BOX, "tag"), QuantileRequest(None, "nosuch"), QuantileRequest("num = ", "qty"), QuantileRequest("tag MATCHES 't[12]'", "qty"),
            QuantileRequest(None, "tag"), QuantileRequest(None, None), QuantileRequest(None, "qty", Q_MEDIAN, "nosuch"), QuantileRequest(None, "qty", Q_MEDIAN, "idx"),
            QuantileRequest(None, "qty", ()), QuantileRequest(None, "qty", tuple(i / 16 for i in range(17))), QuantileRequest(None, "qty", (0.5, -0.1)),
            QuantileRequest(None, "qty", (1.5,)), QuantileRequest(None, "price", (float("nan"),)), QuantileRequest(None, "qty", ("half",)),
            QuantileRequest("num = 3", "big", Q_SIXTEEN, "one")]
    got = e.field_quantiles(reqs)
    for i in (0, 14):
        check(m, got[i], reqs[i])
    for i in range(1, 14):
        assert got[i].error and (got[i].values, got[i].count, got[i].total, got[i].groups) == ([], 0, 0, []), (i, got[i])
    assert "nosuch" in got[1].error and "syntax" in got[2].error and "string" in got[4].error and "4096" in got[7].error and "16" in got[9].error and "[0, 1]" in got[10].error
    assert got[10].q == (0.5, -0.1) and math.isnan(got[13].q[0])
    one = e.field_quantiles(None, "qty", (2,))
    assert one.error and "[0, 1]" in one.error


def test_two_sessions_and_repeated_calls_return_equal_objects(fx):
    e, m = fx
    reqs = [QuantileRequest(f, field, q, g) for f in (None, "num < 20") for field, q, g in (("price", Q_BOX, None), ("price", Q_SIXTEEN, "tag"), ("uniq", Q_BOX, "g3000"),
                                                                                          ("qty", Q_ENDS, "tag"), ("big", Q_MEDIAN, "g1000"))]
    a, b = Session(e), Session(e)
    try:
        first = a.field_quantiles(reqs)
        for s in (a, b, a, b):
            again = s.field_quantiles(reqs)
            assert again == first and repr(again) == repr(first)
        assert [s.field_quantiles(r.filter, r.field, r.q, r.group_by) for s, r in zip((a, b) * 5, reqs)] == first      # one by one, another order of calls
    finally:
        a.close(); b.close()


def test_masks_are_shared_with_field_stats(fx):
    e, m = fx
    s = Session(e)
    try:
        s.field_stats("num < 20", "qty")
        assert s.last_field_stats_stats()[:2] == (1, 0)
        r = QuantileRequest("num < 20", "price", Q_BOX, "tag")
        check(m, s.field_quantiles(r.filter, r.field, r.q, r.group_by), r)
        assert s.last_field_quantiles_stats()[:2] == (0, 1)      # field_stats' mask, reused
        r = QuantileRequest("tag = 't2'", "qty")
        check(m, s.field_quantiles(r.filter, r.field), r)
        assert s.last_field_quantiles_stats() == (1, 0, 1, 3)    # the mask build, one histogram, one pick
        assert s.list_documents("tag = 't2'", None, True, 0, 5).total == s.field_quantiles("tag = 't2'", "qty").total and s.last_list_stats()[:2] == (0, 1)
    finally:
        s.close()


def test_a_deletion_and_a_restore_change_the_answers():
    m = Model()
    e = build(m, ("idx", "num", "g3000", "qty", "price"))
    r = QuantileRequest("num < 20", "price", Q_BOX, "tag")
    before = e.field_quantiles(r.filter, r.field, r.q, r.group_by)
    check(m, before, r)
    gone = np.nonzero(m.members("num < 20") & (m.price > 50))[0][:40]
    assert e.delete_documents(m.keys[gone]) == 40
    m.live[gone] = False
    after = e.field_quantiles(r.filter, r.field, r.q, r.group_by)
    check(m, after, r)
    assert after.total == before.total - 40 and after.values != before.values and e.last_field_quantiles_stats()[:2] == (1, 0)      # the mask was built again
    for q in (QuantileRequest(None, "qty", Q_SIXTEEN, "g3000"), QuantileRequest(None, "qty")):
        check(m, e.field_quantiles(q.filter, q.field, q.q, q.group_by), q)
    e.restore_documents()
    m.live[:] = True
    check(m, e.field_quantiles(r.filter, r.field, r.q, r.group_by), r)


@pytest.mark.parametrize("n", [1, 12, 15, 16, 17, 31])
def test_small_corpora(n):
    """As tests/test_gpu_set_walk.py walks them: less than two groups of 16, every run of accepted documents that begins or ends inside a group of four."""
    shade = (["red", "blue", "green"] * 11)[:n]
    size = np.arange(1, n + 1, dtype=np.int64)
    weight = np.where(size % 5 == 0, np.nan, (size * 7 % 11).astype(np.float64))
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "alpha bravo item %d" % i) for i in range(n)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size); e.set_column("weight", weight)
    filters = ["size >= %d" % v for v in range(1, n + 2)] + ["size <= %d" % v for v in range(1, n)] + ["size = 5", "size = 6 OR size = 11", None]

    def accept(x):
        out = np.zeros(n, bool) if x is not None else np.ones(n, bool)
        for part in (x or "").split(" OR ") if x else []:
            _, op, v = part.split()
            out |= {">=": size >= int(v), "<=": size <= int(v), "=": size == int(v)}[op]
        return out
    for field, col in (("size", size), ("weight", weight)):
        got = e.field_quantiles([QuantileRequest(x, field, Q_BOX, "shade") for x in filters])
        assert len(got) == len(filters)
        for x, a in zip(filters, got):
            acc = accept(x)
            count, nan, vals = Model.figures(col[acc], Q_BOX)
            assert a.error is None and same([a.count, a.nan, a.values], [count, nan, vals]) and a.total == int(acc.sum()), (n, field, x, a, vals)
            want = {s: Model.figures(col[acc & (np.array(shade) == s)], Q_BOX) for s in set(np.array(shade)[acc])}
            assert {g.value: (g.count, g.nan, g.values) for g in a.groups} == want and len(a.groups) == len(want), (n, field, x, a.groups, want)


BIG = 70001


@pytest.fixture(scope="module")
def big():
    """70 001 documents, `wide` of 70 001 values (17 bits of keys), `coarse` of 45, `g7` of seven groups"""
    rng = np.random.default_rng(3)
    e = SearchEngine.create_default(device=0)
    texts = [E._u16("w%d item" % (i % 13)) for i in range(BIG)]
    offs = np.zeros(BIG + 1, np.uint64); offs[1:] = np.cumsum([len(t) for t in texts])
    e.index_flat(None, np.concatenate(texts), offs)
    cols = {"wide": rng.permutation(BIG).astype(np.int64) * 3 - 100000, "coarse": rng.integers(-5, 40, BIG).astype(np.int64), "g7": (np.arange(BIG) % 7).astype(np.int64),
            "num": rng.integers(0, 100, BIG).astype(np.int64)}
    for name, col in cols.items():
        e.set_column(name, col)
    return e, cols


def test_every_digit_width_gives_the_same_answers_and_only_the_pass_count_changes(big):
    e, cols = big
    s = Session(e)
    try:
        reqs = [QuantileRequest(None, "wide", Q_SIXTEEN), QuantileRequest("num < 20", "wide", Q_BOX, "g7"), QuantileRequest("num < 20", "coarse", Q_BOX, "g7")]
        acc = {None: np.ones(BIG, bool), "num < 20": cols["num"] < 20}
        first = s.field_quantiles(reqs)                           # the engine chooses: 17 bits in two passes
        assert s.last_field_quantiles_stats()[2] == 2
        for r, a in zip(reqs, first):
            count, nan, vals = Model.figures(cols[r.field][acc[r.filter]], r.q)
            assert a.error is None and same([a.count, a.nan, a.values], [count, nan, vals]), (r, a)
            if r.group_by:
                want = {str(g): Model.figures(cols[r.field][acc[r.filter] & (cols["g7"] == g)], r.q) for g in range(7)}
                assert {g.value: (g.count, g.nan, g.values) for g in a.groups} == want
        for bits in range(4, 12):
            s.set_quantile_digit_bits(bits)
            assert s.field_quantiles(reqs) == first, bits
            assert s.last_field_quantiles_stats()[2] == -(-17 // bits), bits      # the widest request's passes: ceil(17 / bits) histogram launches, five at 4 bits, two at 11
            assert s.field_quantiles(reqs[2:]) == first[2:] and s.last_field_quantiles_stats()[2] == -(-6 // bits)      # 45 values: 6 bits
        s.set_quantile_digit_bits(0)
        assert s.field_quantiles(reqs) == first and s.last_field_quantiles_stats()[2] == 2
    finally:
        s.close()
