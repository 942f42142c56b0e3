"""Query.pre_filter on the GPU: rank only the documents a filter accepts.

The contract: a query with pre_filter P returns what the same query returns on the same index if every document P does not accept carried
Document.Deleted.  The checks restate that from the test side: the masks against tests/browse_model.py (the oracle's filter VM per document), the
results against the oracle with those documents deleted (oracle delete_keys / restore_all), and against a second engine of the same corpus on which
the rejected documents ARE deleted."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import Session, pack_texts, _install_prefilters, _query_error
from tests import oracle_lib as O
from tests.browse_model import BrowseModel
from tests.parity_classify import assert_final_rows, stage2_scored
from tests.test_gpu_boost_sort import columns, rows_of, assert_rows
from tests.test_gpu_post_rows import DOCS as PLATEAU_DOCS, TEXTS as PLATEAU_TEXTS
from tests.test_gpu_query_options import EXPRS
from tools.synth import Synth

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1027]     # around the four documents of a thread, a wave, a workgroup; several workgroups
NOTHING, EVERYTHING = "year < 1900", "year >= 1900"


def model_of(cols, keys=None):
    year, rating, genre = cols
    return BrowseModel({"year": (year, True), "rating": (rating, False), "genre": (genre, True)}, keys)


def set_columns(x, cols):
    year, rating, genre = cols
    x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)


def expected_mask(model, expr):
    return np.asarray([0 if (d not in model.deleted and model.holds(expr, d)) else 1 for d in range(model.n)], np.uint8)


def flags_of(r):
    return (r.unsupported, r.used_coverage, r.stage1_fallback, r.skipped_candidates)


def once(e, qs):
    """qs through search_queries on a session of its own, closed afterwards."""
    s = Session(e)
    try:
        return s.search_queries(qs)
    finally:
        s.close()


def assert_bits_equal(r, w, ctx):
    assert r.error is None and w.error is None, (ctx, r.error, w.error)
    assert_rows(rows_of(r), rows_of(w), ctx)
    assert flags_of(r) == flags_of(w), ctx


# ---- the mask kernel against the test-side model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_masks_equal_the_model(n):
    cols = columns(n)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(k, "alpha bravo item %d" % k) for k in range(n)])
    set_columns(e, cols)
    model = model_of(cols)
    for deleted in ([], list(range(0, n, 10))):                   # the second round with about a tenth of the documents deleted
        if deleted:
            assert e.delete_document_ids(deleted) == len(deleted)
            model.deleted = set(deleted)
        want = {x: expected_mask(model, x) for x in EXPRS}
        one = Session(e)                                          # one expression per launch: K = 1
        for x in EXPRS:
            got = one.prefilter_mask(x)
            assert one.last_prefilter_stats() == (1, 0, 1), x
            assert got.dtype == np.uint8 and got.shape == (n,) and np.array_equal(got, want[x]), (n, x, np.flatnonzero(got != want[x])[:8])
        many = Session(e)                                         # all 12 in one batch: one launch with K = 12 that reads all three columns
        res = many.search_queries([Query("alpha", 10, pre_filter=x) for x in EXPRS])
        assert many.last_prefilter_stats() == (len(EXPRS), 0, 1)
        for x, r in zip(EXPRS, res):
            assert r.error is None, (x, r.error)
            assert r.total_in_pre_filter == model.count(x) == int((want[x] == 0).sum()), (n, x)
            assert all(want[x][rec.document_id] == 0 for rec in r.records), (n, x)
            got = many.prefilter_mask(x)                          # the batch's mask, from the session's cache
            assert many.last_prefilter_stats() == (0, 1, 0), x
            assert np.array_equal(got, want[x]), (n, x, np.flatnonzero(got != want[x])[:8])
        one.close(); many.close()


# ---- a mixed batch against the oracle with deletions ------------------------------------------------------------------------------------------
# Six pre-filters that accept 7 % - 38 % of the 40 000 documents (2661 .. 15237).  The seed was chosen with the oracle alone, on the CPU: 77 of the 100
# queries carry a pre-filter, all six expressions occur, every pre-filtered query returns rows, 67 return their full max_results and 73 return other keys than
# the same query without its pre-filter (the test asserts the three conditions again before it looks at the engine).
MIX_EXPRS = [EXPRS[i] for i in (0, 1, 3, 5, 7, 10)]
MIX_SEED = 7


def mixed_prefilter_queries(texts, n=100, seed=MIX_SEED):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pre = MIX_EXPRS[int(rng.integers(len(MIX_EXPRS)))] if rng.random() < 0.7 else None
        out.append(Query(texts[i % len(texts)], int(rng.choice([1, 10, 20, 100])), enable_coverage=bool(rng.random() < 0.7), pre_filter=pre))
    return out


def oracle_prefiltered(o, model, qs):
    """The oracle's answer to each pre-filtered query of qs: the search after delete_keys(documents its pre-filter rejects).  {index: result dict}."""
    out = {}
    for x in sorted({q.pre_filter for q in qs if q.pre_filter is not None}):
        rejected = [d for d in range(model.n) if not model.holds(x, d)]
        o.delete_keys(rejected)
        try:
            for i, q in enumerate(qs):
                if q.pre_filter == x:
                    r = o.search(q.text, q.max_number_of_records_to_return, q.coverage_depth, q.enable_coverage)
                    r["stage1_fallback"] = r["used_coverage"] and len(r["keys"]) > 0 and not stage2_scored(o, r)
                    r["stage2_scored"] = stage2_scored(o, r)
                    out[i] = r
        finally:
            o.restore_all()
    return out


def assert_matches_oracle(r, w, ctx):
    assert r.error is None, (ctx, r.error)
    assert [x.document_id for x in r.records] == w["keys"], (ctx, [x.document_id for x in r.records][:12], w["keys"][:12])
    assert [x.tiebreaker for x in r.records] == w["ties"].tolist(), ctx
    assert (r.used_coverage, r.stage1_fallback) == (w["used_coverage"], w["stage1_fallback"]), ctx
    assert_final_rows(w["keys"], [x.score for x in r.records], w["keys"], w["scores"], w["stage2_scored"], ctx)


@pytest.fixture(scope="module")
def fx():
    s = Synth(2, docs=40000)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    cols = columns(40000)
    for x in (e, o):
        set_columns(x, cols)
    qa, qo = s.queries(60, qseed=43, fuzz=0.3)
    return e, o, model_of(cols), Synth.texts(qa, qo)


def test_mixed_batch_equals_the_oracle_with_deletions(fx):
    e, o, model, texts = fx
    qs = mixed_prefilter_queries(texts)
    pre = [i for i, q in enumerate(qs) if q.pre_filter is not None]
    assert 60 <= len(pre) <= 80 and len({qs[i].pre_filter for i in pre}) == len(MIX_EXPRS)
    want = oracle_prefiltered(o, model, qs)
    # the conditions the seed was chosen for, from the oracle alone
    assert sum(1 for i in pre if want[i]["keys"]) >= 0.8 * len(pre)
    assert any(len(want[i]["keys"]) == qs[i].max_number_of_records_to_return for i in pre)
    assert any(want[i]["keys"] != o.search(qs[i].text, qs[i].max_number_of_records_to_return, 500, qs[i].enable_coverage)["keys"] for i in pre)
    s = Session(e)
    res = s.search_queries(qs)
    assert s.last_prefilter_stats() == (len(MIX_EXPRS), 0, 1)      # one launch builds the six masks
    for i in pre:
        assert_matches_oracle(res[i], want[i], (i, qs[i].text, qs[i].pre_filter, qs[i].max_number_of_records_to_return))
        assert res[i].total_in_pre_filter == model.count(qs[i].pre_filter)
    # the queries without a pre-filter: the bits of the same queries in a batch that has no pre-filter at all
    rest = [i for i in range(len(qs)) if i not in pre]
    plain = once(e, [qs[i] for i in rest])
    for i, w in zip(rest, plain):
        assert_bits_equal(res[i], w, (i, qs[i].text))
        assert res[i].total_in_pre_filter == 0
    again = s.search_queries(qs)                                   # the masks are reused
    assert s.last_prefilter_stats() == (0, len(MIX_EXPRS), 0)
    for a, b in zip(again, res):
        assert_bits_equal(a, b, "repeat")
    s.close()


def test_extremes(fx):
    e, o, model, texts = fx
    s = Session(e)
    none = s.search_queries([Query(t, 20, pre_filter=NOTHING) for t in texts[:8]])
    for r in none:
        assert r.records == [] and r.error is None and r.total_in_pre_filter == 0
    qs = [Query(t, 20, enable_coverage=(i % 2 == 0)) for i, t in enumerate(texts[:8])]
    plain = s.search_queries(qs)
    every = s.search_queries([Query(q.text, 20, enable_coverage=q.enable_coverage, pre_filter=EVERYTHING) for q in qs])
    for r, w in zip(every, plain):
        assert_bits_equal(r, w, "everything")
        assert r.total_in_pre_filter == model.n
    s.close()


def test_two_sessions_on_two_threads(fx):
    e, o, model, texts = fx
    batches = [[Query(t, 20, pre_filter=MIX_EXPRS[0]) for t in texts[:30]], [Query(t, 20, pre_filter=MIX_EXPRS[2]) for t in texts[:30]]]
    seq = [once(e, b) for b in batches]
    out, err = [None, None], []

    def run(k):
        try:
            s = Session(e)
            try:
                for _ in range(3):
                    out[k] = s.search_queries(batches[k])
            finally:
                s.close()
        except Exception as x:                                     # pragma: no cover
            err.append(x)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k in range(2):
        for r, w in zip(out[k], seq[k]):
            assert_bits_equal(r, w, k)
            assert r.total_in_pre_filter == w.total_in_pre_filter == model.count(batches[k][0].pre_filter)


# ---- the plateau corpus: the exact replay decides the cut ---------------------------------------------------------------------------------------
PLATEAU_EXPRS = ["year >= 1960 AND genre != 'Horror'", "rating > 5.5 AND rating < 8.5", "year BETWEEN 1990 AND 1999"]


@pytest.fixture(scope="module")
def plateau():
    n = len(PLATEAU_DOCS)
    cols = columns(n)
    e = SearchEngine.create_default(device=0); e.index_documents([Document(k, t) for k, t in PLATEAU_DOCS])
    o = O.OracleEngine.create_default(); o.index(PLATEAU_DOCS)
    for x in (e, o):
        set_columns(x, cols)
    return e, o, cols, model_of(cols)


def test_plateau_replay_reads_the_mask(plateau):
    e, o, cols, model = plateau
    qs = [Query(t, k, 500, cov, pre_filter=x) for x in PLATEAU_EXPRS for t in PLATEAU_TEXTS for k, cov in ((20, True), (20, False))]
    want = oracle_prefiltered(o, model, qs)
    replays = 0
    for x in PLATEAU_EXPRS:                                        # one batch per pre-filter: every query of a batch that replays is pre-filtered
        idx = [i for i, q in enumerate(qs) if q.pre_filter == x]
        res = e.search_queries([qs[i] for i in idx])
        replays += e.last_timings()["exact_replays"]
        for i, r in zip(idx, res):
            assert_matches_oracle(r, want[i], (qs[i].text, x, qs[i].enable_coverage))
    assert replays > 0


# ---- engine against itself: the rejected documents really deleted, duplicate keys allowed ---------------------------------------------------------
@pytest.fixture(scope="module")
def twins():
    n = len(PLATEAU_DOCS)
    cols = columns(n, seed=9)
    docs = [Document(k // 2, t) for k, t in PLATEAU_DOCS]          # two documents per key: the mask is per document, not per key
    out = []
    for _ in range(2):
        e = SearchEngine.create_default(device=0); e.index_documents(docs); set_columns(e, cols)
        out.append(e)
    return out[0], out[1], model_of(cols, [d.document_key for d in docs])


def delete_rejected(b, model, expr):
    b.restore_documents()
    rejected = [d for d in range(model.n) if not model.holds(expr, d)]
    if rejected:
        b.delete_document_ids(rejected)


def test_prefilter_equals_deleting_the_rejected_documents(twins):
    a, b, model = twins
    for x in PLATEAU_EXPRS + [EXPRS[1], EXPRS[7]]:
        delete_rejected(b, model, x)
        for k, depth, cov in ((20, 500, True), (100, 500, False), (64, 200, True)):
            got = a.search_queries([Query(t, k, depth, cov, pre_filter=x) for t in PLATEAU_TEXTS])
            want = b.search_queries([Query(t, k, depth, cov) for t in PLATEAU_TEXTS])
            for r, w in zip(got, want):
                assert_bits_equal(r, w, (x, k, depth, cov))
                assert len(w.records) > 0
    b.restore_documents()


def test_prefilter_then_post_processing(twins):
    a, b, model = twins
    pre, flt = PLATEAU_EXPRS[0], "rating > 3.0"
    boosts = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low)]
    opts = dict(filter=flt, enable_facets=True, enable_boost=True, boosts=boosts, sort_by="rating", sort_ascending=True)
    delete_rejected(b, model, pre)
    try:
        got = a.search_queries([Query(t, 50, **opts, pre_filter=pre) for t in PLATEAU_TEXTS])
        want = b.search_queries([Query(t, 50, **opts) for t in PLATEAU_TEXTS])
        for r, w in zip(got, want):
            assert_bits_equal(r, w, "post")
            assert len(w.records) > 0 and r.facets == w.facets
        # total_in_filter is unchanged by a pre-filter: engine A's own count, with nothing deleted
        own = a.search_queries([Query(PLATEAU_TEXTS[0], 50, filter=flt)])[0]
        assert all(r.total_in_filter == own.total_in_filter == model.count(flt) for r in got)
        # the session-wide path with one pre-filter for the batch
        sw = a.search_filtered(PLATEAU_TEXTS, 50, **{k: v for k, v in opts.items()}, pre_filter=pre)
        for r, w in zip(sw, got):
            assert_bits_equal(r, w, "search_filtered")
            assert r.facets == w.facets and r.total_in_pre_filter == w.total_in_pre_filter == model.count(pre)
        single = a.search(Query(PLATEAU_TEXTS[0], 50, **opts, pre_filter=pre))
        assert_bits_equal(single, got[0], "search")
    finally:
        b.restore_documents()


# ---- invalidation ------------------------------------------------------------------------------------------------------------------------------
def test_masks_follow_deletions_and_new_columns():
    docs = [Document(k, "alpha bravo %d" % k) for k in range(1, 9)]
    year = np.array([1990, 1995, 2000, 2005, 2010, 2015, 2020, 2025], np.int64)
    e = SearchEngine.create_default(device=0); e.index_documents(docs); e.set_column("year", year, facetable=True)
    o = O.OracleEngine.create_default(); o.index([(d.document_key, d.fields) for d in docs])
    q = [Query("alpha", 10, pre_filter="year >= 2000"), Query("alpha", 10)]

    def check(deleted, built):
        o.restore_all(); o.delete_keys([1, 2] + deleted)           # keys 1, 2: year < 2000
        w = o.search("alpha", 10)
        r = e.search_queries(q)
        assert e.last_prefilter_stats() == ((1, 0, 1) if built else (0, 1, 0))
        assert [x.document_id for x in r[0].records] == w["keys"] and len(w["keys"]) == 6 - len(deleted)
        assert r[0].total_in_pre_filter == 6 - len(deleted)
        o.restore_all(); o.delete_keys(deleted) if deleted else None
        assert [x.document_id for x in r[1].records] == o.search("alpha", 10)["keys"]
    check([], True)
    check([], False)                                              # a repeated batch with no change: reused
    e.delete_documents([3, 8])
    check([3, 8], True)
    check([3, 8], False)
    e.restore_documents()
    check([], True)
    e.delete_document_ids([4])                                    # internal id 4 = key 5
    check([5], True)
    e.restore_documents()
    check([], True)
    e.set_column("shelf", np.array([1, 2, 1, 2, 1, 2, 1, 2], np.int64))      # a column made after first use: a new epoch, the expression compiled again
    check([], True)
    r = e.search_queries([Query("alpha", 10, pre_filter="shelf = 2 AND year >= 2000")])[0]
    assert sorted(x.document_id for x in r.records) == [4, 6, 8] and r.total_in_pre_filter == 3


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refused_queries_leave_their_neighbours_alone(fx):
    e, o, model, texts = fx
    good = [Query(t, 10, pre_filter=MIX_EXPRS[i % 3] if i % 2 else None) for i, t in enumerate(texts[:12])]
    bad = [(Query(texts[0], 10, pre_filter="year >= "), 1), (Query(texts[1], 10, pre_filter="genre MATCHES '^D'"), 5),
           (Query("", 10, enable_facets=True, pre_filter=MIX_EXPRS[0]), 5)]      # syntax error, MATCHES, a browse query
    pos = [2, 7, 11]
    mixed = list(good)
    for p, (b, _) in zip(pos, bad):
        mixed.insert(p, b)
    s = Session(e)
    res = s.search_queries(mixed)
    want = once(e, good)
    for r, w in zip([r for i, r in enumerate(res) if i not in pos], want):
        assert_bits_equal(r, w, "neighbour")
        assert r.total_in_pre_filter == w.total_in_pre_filter
    for p in pos:
        assert res[p].records == [] and res[p].error and res[p].total_in_pre_filter == 0, (p, res[p])
    assert "syntax" in res[2].error and "MATCHES" in res[7].error and "browse" in res[11].error
    # the raw statuses and flags
    st = _install_prefilters(e, s.h, [q.pre_filter for q in mixed])
    assert [int(st[p]) for p in pos] == [1, 5, 0]                  # (the browse query is known when the batch runs)
    assert all(int(x) == 0 for i, x in enumerate(st) if i not in pos)
    keys, scores, ties, counts, flags = s.search_packed(*pack_texts([q.text for q in mixed]), 10, 500, True)
    for p in pos[:2]:
        assert counts[p] == 0 and flags[p] & 16
    assert not any(flags[i] & 16 for i in range(len(mixed)) if i not in pos)
    assert "syntax" in _query_error(e, s.h, 2, 0) and "MATCHES" in _query_error(e, s.h, 7, 0)      # the messages without query options, too
    # a batch of another size fails and clears the pre-filters
    _install_prefilters(e, s.h, [MIX_EXPRS[0]] * 3)
    with pytest.raises(Exception):
        s.search_packed(*pack_texts(texts[:2]), 10, 500, True)
    k2 = s.search_packed(*pack_texts(texts[:3]), 10, 500, True)
    plain = e.search_batch(texts[:3], 10)
    for i in range(3):
        assert [int(k) for k in k2[0][i, :int(k2[3][i])]] == [x.document_id for x in plain[i].records]
    s.close()


def test_a_refusal_reports_its_own_message(fx):
    """search_filtered(pre_filter=) runs without per-query options: the message of a refused pre-filter is its own, not one an earlier per-query batch of
    the same size left on the session."""
    e, o, model, texts = fx
    s = Session(e)
    first = s.search_queries([Query(texts[0], 10, filter="genre MATCHES '^D'"), Query(texts[1], 10)])
    assert first[0].error and "MATCHES" in first[0].error
    r = e.search_filtered(texts[:2], 10, pre_filter="year >= ", session=s)
    assert all(x.records == [] and x.error and "syntax" in x.error and "MATCHES" not in x.error for x in r), [x.error for x in r]
    ok = e.search_filtered(texts[:2], 10, pre_filter=MIX_EXPRS[1], session=s)
    assert all(x.error is None for x in ok) and any(x.records for x in ok)
    s.close()


def test_seventeen_distinct_prefilters(fx):
    e, o, model, texts = fx
    exprs = ["year >= %d" % (1950 + 4 * j) for j in range(17)]
    s = Session(e)
    st = _install_prefilters(e, s.h, exprs + [exprs[0]])
    assert [int(x) for x in st] == [0] * 16 + [4, 0]                # INFX_ECAPACITY on the surplus only
    keys, scores, ties, counts, flags = s.search_packed(*pack_texts([texts[j % len(texts)] for j in range(18)]), 10, 500, True)
    assert counts[16] == 0 and flags[16] & 16 and not any(flags[i] & 16 for i in range(18) if i != 16)
    assert "INFX_MAX_PREFILTERS" in _query_error(e, s.h, 16, 0)
    res = s.search_queries([Query(texts[j % len(texts)], 10, pre_filter=x) for j, x in enumerate(exprs)])     # split into two device batches: all answered
    for x, r in zip(exprs, res):
        assert r.error is None and r.total_in_pre_filter == model.count(x), x
        assert all(model.holds(x, rec.document_id) for rec in r.records)
    assert any(r.records for r in res)
    s.close()


def test_shards_refuse_prefilters():
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_search_queries
    docs = [Document(k, "alpha bravo %d" % k) for k in range(40)]
    year = np.arange(40, dtype=np.int64) + 1980
    engs = [create_sharded_engine(r, 2, 0) for r in range(2)]
    for x in engs:
        x.index_documents(docs); x.set_column("year", year, facetable=True)
    qs = [Query("alpha", 10), Query("alpha", 10, pre_filter="year >= 2000"), Query("bravo 7", 5)]
    got = simulate_search_queries([ShardSession(x) for x in engs], qs)
    assert got[1].records == [] and got[1].error and "shard" in got[1].error
    u = SearchEngine.create_default(device=0); u.index_documents(docs)
    for r, w in zip((got[0], got[2]), u.search_queries([qs[0], qs[2]])):
        assert_bits_equal(r, w, "shard neighbour")


def test_host_phases_refuse_prefilters():
    script = r'''
import numpy as np
from infidex_amd import SearchEngine, Document, Query
e = SearchEngine.create_default(device=0)
e.index_documents([Document(k, "alpha bravo %d" % k) for k in range(40)])
e.set_column("year", np.arange(40, dtype=np.int64) + 1980, facetable=True)
r = e.search_queries([Query("alpha", 10), Query("alpha", 10, pre_filter="year >= 2000")])
assert r[0].error is None and len(r[0].records) == 10, r[0]
assert r[1].records == [] and r[1].error and "INFX_PHASED" in r[1].error, r[1]
'''
    env = dict(os.environ); env["INFX_PHASED"] = "1"
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", script], check=True, env=env, timeout=300)
