"""Generated Infiscript programs (tests/filter_fuzz.py) on every kernel that runs filt_eval_codes: k_filter_mask_multi, k_filter_count_multi,
k_facets_filtered, k_postfilter / k_postfilter_wide, k_postproc / k_postproc_wide (boost programs) and k_browse_scan.

Corpus: 1027 documents "alpha bravo item %d" (the last group of four is partial) with the columns of filter_fuzz.columns — an int column whose values carry
the codes 0, 31, 32, 33, 63, 64 and 999 of a 1000-value dictionary at known documents, a double column with NaN, -0.0 / +0.0, 1e15, 1e-5, a string column
with mixed case, "", numeric-looking strings and the scripts the case folding now covers — on a default engine and on one with max_post_rows = 1024; every
check runs a second time with every tenth document deleted.

  masks and counts   96 expressions — among them stack depth exactly 32, 255 and 256 ops, literal operands, one leaf per chosen code — against
                     BrowseModel.holds (the oracle's filter VM per document), element for element: one mask per launch, then sixteen per launch.
  row paths          per group of sixteen expressions the engines get sixteen int columns v0..v15, vK = the model's verdict of expression K; every call
                     made with expression K must return, bit for bit, what the same call returns with `vK = 1` — a one-leaf program that
                     tests/test_gpu_filter.py and tests/test_gpu_boost_sort.py hold to the oracle.
  refusals           depth 33 and 257 ops are refused per query / per expression with check_filter_prog's message, like a syntax error.
  many columns       11 and 64 columns read by one expression: the one-wave launches, and at 64 columns the raised dynamic-LDS limit — of the mask and
                     facet kernels, and of k_filter_count_multi and k_browse_scan, whose sixteen programs over 64 columns need 65 600 bytes.

What a wrong kernel would show: reading table word `c >> 6` instead of `c >> 5` moves the chosen codes 32, 33, 63, 64 and 999 to other words, so the
single-leaf masks fail; a TERN that pops one entry too few leaves its condition under the result, which the enclosing OR of the depth-32 ternary chain then
reads as its left operand; a stack with fewer than 32 entries drops operands of the chains at depth 9, 16, 17, 31 and 32, each of which decides a document
of its own (tests/test_filter_model.py replays them through a loop with every smaller capacity); a 255- or 256-op program cut short loses the documents of
the leaves it never reached; a one-wave launch whose LDS is sized or indexed for 256 threads either fails to launch at 64 columns ((64 * 4 * 256 + 16) * 4 =
262 208 bytes) or reads slots no lane wrote at 11.  NOT observable here: the `c < L.num_values` guard — a code that encode_column made is always below
num_values, and a field no column has reads code 0 of a one-value table."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import Session, InfidexError
from tests import filter_fuzz as FZ
from tests.browse_model import BrowseModel, order_facets, facet_text
from tests.test_gpu_boost_sort import rows_of, assert_rows

pytestmark = pytest.mark.gpu

N = 1027
SEED, COUNT, GROUP = 10, 96, 16                  # the seed of tests/test_filter_model.py: its first 96 programs' trees, printed with other spellings
DOCS = [Document(k, "alpha bravo item %d" % k) for k in range(N)]
DELETED = list(range(0, N, 10))


def make_engine(cols, n=N, **kw):
    e = SearchEngine.create_default(device=0, **kw)
    e.index_documents(DOCS[:n])
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    return e


class Env:
    def __init__(self):
        self.trees, self.exprs = FZ.generate(SEED, COUNT)
        self.cols = FZ.columns(N)
        self.model = BrowseModel(self.cols)
        # the model's verdict of every expression on every document, computed once (Deleted not looked at) and left unchanged
        self.verdict = np.asarray([[bool(self.model.holds(x, d)) for d in range(N)] for x in self.exprs], bool)
        self.live = np.ones(N, bool)

    def count(self, k):
        return int((self.verdict[k] & self.live).sum())

    def mask(self, k):
        return np.where(self.verdict[k] & self.live, 0, 1).astype(np.uint8)


@pytest.fixture(scope="module")
def env():
    return Env()


def test_the_programs_reach_the_limits(env):
    shapes = [(FZ.ops(t), FZ.depth(t)) for t in env.trees]
    assert sum(d == 32 for _, d in shapes) == 3 and (255, 2) in shapes and (256, 2) in shapes and max(d for _, d in shapes) == 32
    assert {9, 16, 17, 31} <= {d for _, d in shapes}
    assert set().union(*(FZ.kinds(t) for t in env.trees)) == {"leaf", "ne", "lit", "not", "and", "or", "tern"}
    for c, t in zip(FZ.CHOSEN_CODES, FZ.code_leaves()):                     # a leaf per chosen code: exactly the documents that carry the code
        k = env.trees.index(t)
        assert np.flatnonzero(env.verdict[k]).tolist() == [d for d in range(N) if env.cols[FZ.INT][0][d] == FZ.INT_VALUES[c]] and env.verdict[k][c]
    rate = env.verdict.mean(axis=1)
    assert ((rate[:FZ.N_FIXED] > 0) & (rate[:FZ.N_FIXED] < 1)).all(), rate[:FZ.N_FIXED]      # no limit program is constant: every one can fail both ways
    qty = env.cols[FZ.INT][0]                                               # the depth-32 chains: exactly the documents that carry one of the 32 codes
    assert np.array_equal(env.verdict[0], np.isin(qty, [FZ.INT_VALUES[(31 * i) % 1000] for i in range(32)])) and env.verdict[0].sum() >= 32
    assert np.array_equal(~env.verdict[1], np.isin(qty, [FZ.INT_VALUES[(7 + 29 * i) % 1000] for i in range(32)])) and (~env.verdict[1]).sum() >= 32
    assert int(((rate >= 0.05) & (rate <= 0.95)).sum()) >= 40, rate


# ---- C1: masks and counts against the model ---------------------------------------------------------------------------------------------------------
def test_masks_and_counts_equal_the_model(env):
    e = make_engine(env.cols)
    try:
        for deleted in ([], DELETED):
            if deleted:
                assert e.delete_document_ids(deleted) == len(deleted)
                env.live[deleted] = False
            one = Session(e)                                                # one expression per launch: K = 1
            for k, x in enumerate(env.exprs):
                got = one.prefilter_mask(x)
                assert one.last_prefilter_stats() == (1, 0, 1), x
                assert got.dtype == np.uint8 and got.shape == (N,) and np.array_equal(got, env.mask(k)), (k, x[:200], np.flatnonzero(got != env.mask(k))[:8])
            one.close()
            for g in range(0, COUNT, GROUP):                                # sixteen per launch: K = 16
                many = Session(e)
                xs = env.exprs[g:g + GROUP]
                res = many.search_queries([Query("alpha", 10, pre_filter=x) for x in xs])
                assert many.last_prefilter_stats() == (GROUP, 0, 1)
                flt = many.search_queries([Query("alpha", 10, filter=x) for x in xs])      # NumberOfDocumentsInFilter: k_filter_count_multi with K = 16
                if not deleted:
                    assert many.last_count_stats() == (GROUP, 1)
                fac = many.facets_of_documents(xs)
                for j, x in enumerate(xs):
                    k = g + j
                    assert res[j].error is None and flt[j].error is None and fac[j].error is None, (x[:200], res[j].error, flt[j].error, fac[j].error)
                    got = many.prefilter_mask(x)                            # the batch's mask, from the session's cache
                    assert many.last_prefilter_stats() == (0, 1, 0), x
                    assert np.array_equal(got, env.mask(k)), (k, x[:200], np.flatnonzero(got != env.mask(k))[:8])
                    assert res[j].total_in_pre_filter == flt[j].total_in_filter == fac[j].total == env.count(k), \
                        (k, x[:200], res[j].total_in_pre_filter, flt[j].total_in_filter, fac[j].total, env.count(k))
                    assert all(env.verdict[k][r.document_id] for r in res[j].records) and all(env.verdict[k][r.document_id] for r in flt[j].records)
                many.close()
    finally:
        env.live[:] = True
        e.close()


# ---- C2: row paths against a verdict column -------------------------------------------------------------------------------------------------------------
def flags_of(r):
    return (r.unsupported, r.used_coverage, r.stage1_fallback, r.skipped_candidates)


def assert_same(r, w, ctx):
    assert r.error is None and w.error is None, (ctx, r.error, w.error)
    assert_rows(rows_of(r), rows_of(w), ctx)
    assert flags_of(r) == flags_of(w), ctx
    assert r.facets == w.facets, (ctx, r.facets, w.facets)
    assert (r.total_in_filter, r.total_in_pre_filter) == (w.total_in_filter, w.total_in_pre_filter), (ctx, r.total_in_filter, w.total_in_filter, r.total_in_pre_filter, w.total_in_pre_filter)
    assert r.pre_filter_facets == w.pre_filter_facets, ctx


def row_queries(f, other, wide):
    """The calls of one expression f (other: a second one, the filter beside a boost): (name, Query)."""
    strong, weak = [Boost(f, BoostStrength.High)], [Boost(f, BoostStrength.Low), Boost(other, BoostStrength.Med)]
    if wide:
        return [("filter 300", Query("alpha", 300, 500, False, filter=f, enable_facets=True)),
                ("filter 1024", Query("alpha", 1024, 1024, False, filter=f, enable_facets=True)),
                ("boost 300", Query("alpha", 300, 500, False, enable_boost=True, boosts=strong)),
                ("boost + filter 300", Query("alpha", 300, 500, False, filter=other, enable_facets=True, enable_boost=True, boosts=weak)),
                ("browse 100", Query("", 100, filter=f, enable_facets=True))]
    return [("filter 64", Query("alpha", 64, filter=f, enable_facets=True)),
            ("boost 64", Query("alpha", 64, enable_boost=True, boosts=strong)),
            ("boost + filter 64", Query("alpha", 64, filter=other, enable_facets=True, enable_boost=True, boosts=weak)),
            ("browse 64", Query("", 64, filter=f, enable_facets=True)),
            ("pre-filter", Query("alpha", 20, pre_filter=f, pre_filter_facets=True))]


@pytest.mark.parametrize("group", range(COUNT // GROUP))
def test_row_paths_equal_a_verdict_column(env, group):
    g = group * GROUP
    xs = env.exprs[g:g + GROUP]
    vs = ["v%d = 1" % j for j in range(GROUP)]
    cols = dict(env.cols)
    for j in range(GROUP):
        cols["v%d" % j] = (env.verdict[g + j].astype(np.int64), False)
    model = BrowseModel(cols)
    narrow, wide = make_engine(cols), make_engine(cols, max_post_rows=1024, max_depth=1024)
    try:
        for deleted in ([], DELETED):
            if deleted:
                for e in (narrow, wide):
                    assert e.delete_document_ids(deleted) == len(deleted)
                model.deleted = set(deleted)
            kept = 0
            for e, is_wide in ((narrow, False), (wide, True)):
                names, got, want = [], [], []
                for j in range(GROUP):
                    o = (j + 5) % GROUP
                    for (name, q), (_, w) in zip(row_queries(xs[j], xs[o], is_wide), row_queries(vs[j], vs[o], is_wide)):
                        names.append((j, name)); got.append(q); want.append(w)
                s = Session(e)
                rg = s.search_queries(got)
                rw = s.search_queries(want)
                s.close()
                for (j, name), q, r, w in zip(names, got, rg, rw):
                    assert_same(r, w, (deleted[:2], j, name, xs[j][:200]))
                    if name.startswith("browse"):                           # ... and the browse rows against the model's own walk
                        model.check(r, vs[j], q.max_number_of_records_to_return, (j, name))
                    kept += len(r.records)
                # without post-processing the base query returns every row asked for: the filters had rows to keep and to drop
                base = e.search_queries([Query("alpha", 1024, 1024, False)] if is_wide else [Query("alpha", 64)])[0]
                assert len(base.records) == min(1024 if is_wide else 64, N - len(deleted))
                fg, fw = e.facets_of_documents(xs), e.facets_of_documents(vs)      # all sixteen at once
                for j in range(GROUP):
                    assert fg[j] == fw[j] and fg[j].error is None, (deleted[:2], j, xs[j][:200], fg[j].total, fw[j].total)
                    assert fg[j].total == int((env.verdict[g + j] & ~np.isin(np.arange(N), deleted)).sum())
            assert kept > 1000
    finally:
        narrow.close(); wide.close()


# ---- C3: refusals ------------------------------------------------------------------------------------------------------------------------------------------
TOO_DEEP, TOO_LONG = "too deeply nested filter program", "filter program too long"      # check_filter_prog's messages


def test_programs_over_the_limits_are_refused(env):
    pool = FZ.leaf_pool(np.random.default_rng(SEED))
    deep, long_ = (FZ.text(t) for t in FZ.over_limit_trees(pool))
    e = make_engine(env.cols)
    rate = env.verdict.mean(axis=1)
    gi = [k for k in range(FZ.N_FIXED, COUNT) if 0.6 <= rate[k] <= 0.98][:3]            # three generated expressions that keep most rows
    good = [env.exprs[k] for k in gi]
    try:
        s = Session(e)
        alone = s.search_queries([Query("alpha", 10, filter=good[0], enable_facets=True), Query("alpha", 10, pre_filter=good[1]), Query("", 10, filter=good[2], enable_facets=True)])
        for bad, why in ((deep, TOO_DEEP), (long_, TOO_LONG)):
            # the session-wide paths raise, as for a syntax error
            for q in (Query("alpha", 10, filter=bad), Query("alpha", 10, enable_boost=True, boosts=[Boost(bad, BoostStrength.Med)]), Query("", 10, filter=bad, enable_facets=True)):
                with pytest.raises(InfidexError, match=why):
                    e.search(q)
            with pytest.raises(InfidexError, match=why):
                s.prefilter_mask(bad)
            # per query: the refused ones come back empty with the message, their neighbours as they do alone
            batch = [Query("alpha", 10, filter=good[0], enable_facets=True), Query("alpha", 10, filter=bad, enable_facets=True),
                     Query("alpha", 10, pre_filter=good[1]), Query("alpha", 10, enable_boost=True, boosts=[Boost(good[0], 1), Boost(bad, 2)]),
                     Query("alpha", 10, pre_filter=bad, pre_filter_facets=True), Query("", 10, filter=bad, enable_facets=True), Query("", 10, filter=good[2], enable_facets=True)]
            res = s.search_queries(batch)
            for i in (1, 3, 4, 5):
                assert res[i].records == [] and res[i].error and why in res[i].error, (i, res[i].error)
                assert res[i].facets is None and res[i].pre_filter_facets is None and res[i].total_in_filter == 0 and res[i].total_in_pre_filter == 0
            for i, w in zip((0, 2, 6), alone):
                assert_same(res[i], w, ("neighbour", i))
            assert len(alone[1].records) == 10 and len(alone[2].records) == 10
            ff = s.facets_of_documents([good[0], bad, good[1]])
            assert ff[1].error and why in ff[1].error and ff[1].facets == {} and ff[1].total == 0
            assert ff[0].error is None and ff[2].error is None and ff[0].total == env.count(gi[0]) and ff[2].total == env.count(gi[1])
            one = s.facets_of_documents(bad)
            assert one.error == ff[1].error
            # the session answers a valid expression afterwards
            assert np.array_equal(s.prefilter_mask(good[2]), env.mask(gi[2]))
            again = s.search_queries([Query("alpha", 10, filter=good[0], enable_facets=True)])[0]
            assert_same(again, alone[0], "afterwards")
        s.close()
    finally:
        e.close()


# ---- C4: many columns ------------------------------------------------------------------------------------------------------------------------------------------
def many_columns(m, n):
    """m int columns: document d carries 1 in column d % (m + 1) alone (none when that is m), other small values elsewhere; the first eight are facetable."""
    cols = {}
    for j in range(m):
        cols["c%d" % j] = (np.asarray([1 if d % (m + 1) == j else 2 + (d * 7 + j * 3 + d // 5) % 4 for d in range(n)], np.int64), j < 8)
    return cols


def many_exprs(m):
    every = " OR ".join("c%d = 1" % j for j in range(m))                    # reads all m columns
    return [every, "c0 = 1", "c%d = 1" % (m - 1), "c%d != 1 AND c%d > 2" % (m // 2, m - 2), "NOT (%s)" % every, "c1 = 1 OR c%d = 1 OR c%d = 1" % (m // 2, m - 1),
            "c3 IN (2, 3) AND c%d >= 4" % (m - 3), "c%d = 1 ? c0 = 2 : c1 >= 3" % (m - 1), "c2 BETWEEN 2 AND 3", "c%d < 4 AND c%d > 1" % (m - 1, m - 2), "c4 = 5 OR c5 = 5",
            "c6 != 2", "c7 = 1 OR c8 = 1 OR c9 = 1 OR c10 = 1", "c%d IS NOT NULL AND c0 < 5" % (m - 1), "nosuch IS NULL AND c%d = 3" % (m // 3), "c%d >= 0" % (m - 1)]


@pytest.mark.parametrize("n", [3, 257, 1027])
@pytest.mark.parametrize("m", [11, 64])
def test_many_columns(m, n):
    cols = many_columns(m, n)
    exprs = many_exprs(m)
    assert len(exprs) == 16
    model = BrowseModel(cols)
    accept = np.asarray([[bool(model.holds(x, d)) for d in range(n)] for x in exprs], bool)
    assert accept[0].sum() == sum(1 for d in range(n) if d % (m + 1) < m) and (n < 100 or (accept.any(axis=1).all() and not accept[:15].all(axis=1).any()))
    e = make_engine(cols, n)
    try:
        for deleted in ([], list(range(0, n, 10)) if n > 3 else [1]):
            if deleted:
                assert e.delete_document_ids(deleted) == len(deleted)
            live = ~np.isin(np.arange(n), deleted)
            s = Session(e)
            res = s.search_queries([Query("alpha", 10, pre_filter=x) for x in exprs])      # one launch, K = 16, every column read
            assert s.last_prefilter_stats() == (16, 0, 1)
            fac = s.facets_of_documents(exprs)
            assert s.last_filtered_facet_stats() == (16, 0, 1)
            for k, x in enumerate(exprs):
                want = np.where(accept[k] & live, 0, 1).astype(np.uint8)
                got = s.prefilter_mask(x)
                assert s.last_prefilter_stats() == (0, 1, 0)
                assert np.array_equal(got, want), (m, n, x[:80], np.flatnonzero(got != want)[:8])
                assert res[k].error is None and res[k].total_in_pre_filter == int((want == 0).sum()), (m, n, x[:80])
                facets = {}
                for name, (vals, facetable) in cols.items():
                    if facetable:
                        c = {}
                        for d in np.flatnonzero(want == 0):
                            c[facet_text(vals[d])] = c.get(facet_text(vals[d]), 0) + 1
                        if c:
                            facets[name] = order_facets(c)
                assert fac[k].error is None and fac[k].total == int((want == 0).sum()) and fac[k].facets == facets, (m, n, x[:80], fac[k].total, fac[k].facets, facets)
            if m == 64 and not deleted:
                # k_filter_count_multi and k_browse_scan with K = 16 over 64 columns: (16 + 64 * 256) * 4 = 65 600 bytes of LDS, past the 64 KiB default limit
                cnt = s.search_queries([Query("alpha", 10, filter=x) for x in exprs])
                assert s.last_count_stats() == (16, 1)
                brw = s.search_queries([Query("", 10, filter=x, enable_facets=True) for x in exprs])
                assert e.last_browse_stats(s) == (16, 1)                    # sixteen groups (their counts are cached by now), one scan launch
                for k, x in enumerate(exprs):
                    assert cnt[k].error is None and cnt[k].total_in_filter == int(accept[k].sum()), (n, x[:80], cnt[k].total_in_filter)
                    assert model.check(brw[k], x, 10, (n, x[:80])) == np.flatnonzero(accept[k])[:10].tolist()      # the first ten accepted documents, in internal order
            alone = Session(e)                                             # the expression that reads every column, alone in its launch
            want = np.where(accept[0] & live, 0, 1).astype(np.uint8)
            assert np.array_equal(alone.prefilter_mask(exprs[0]), want) and alone.last_prefilter_stats() == (1, 0, 1)
            alone.close(); s.close()
    finally:
        e.close()


# ---- facet tie order and sort-by follow the case folding ---------------------------------------------------------------------------------------------------
def test_facet_tie_order_and_sort_by_follow_the_folding():
    """Six values that tie at one document each, whose order under the invariant upper-case table is neither ordinal nor str.lower()'s (filter_fuzz.FOLD_ORDER):
    the facet list of the returned rows, of the accepted documents and of all documents, and the rows of sort_by."""
    vals = [FZ.FOLD_ORDER[i] for i in (3, 1, 5, 2, 4, 0)]
    e = SearchEngine.create_default(device=0)
    try:
        e.index_documents([Document(k, "alpha item %d" % k) for k in range(6)])
        e.set_column("tag", vals, facetable=True)
        want = [(v, 1) for v in FZ.FOLD_ORDER]
        r = e.search(Query("alpha", 10, enable_facets=True))
        assert len(r.records) == 6 and r.facets == {"tag": want}, r.facets
        assert e.facets_of_all_documents() == {"tag": want} and e.facets_of_documents("tag IS NOT NULL").facets == {"tag": want}
        asc = e.search(Query("alpha", 10, sort_by="tag", sort_ascending=True))
        desc = e.search(Query("alpha", 10, sort_by="tag", sort_ascending=False))
        assert [vals[x.document_id] for x in asc.records] == FZ.FOLD_ORDER and [vals[x.document_id] for x in desc.records] == FZ.FOLD_ORDER[::-1]
    finally:
        e.close()
