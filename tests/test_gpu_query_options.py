"""Per-query options on the GPU (infx_engine_set_query_options): a batch of Query objects, each with its own MaxNumberOfRecordsToReturn,
EnableCoverage, Filter, EnableFacets, Boosts and SortBy.  Every query of a mixed batch must return what the same query returns alone through the
session-wide path (test_gpu_filter / test_gpu_boost_sort hold that path to the oracle and to tests/bcl_sort.py); refused queries come back empty
on their own; NumberOfDocumentsInFilter of the expressions a batch uses first is counted in one k_filter_count_multi launch."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import InfidexError, Session, pack_texts, _install_query_options
from tests import oracle_lib as O
from tests.test_gpu_boost_sort import columns, rows_of, assert_rows
from tools.synth import Synth

pytestmark = pytest.mark.gpu

EXPRS = ["year >= 2000 AND rating > 7.0", "genre IN ('Drama', 'crime') OR year < 1960", "NOT (rating <= 5) AND genre != 'Horror'",
         "year BETWEEN 1990 AND 1999", "genre STARTS WITH 'S' OR genre LIKE '%er'", "rating >= 9.5 ? genre = 'Action' : year >= 2020",
         "rating = 7", "nosuchfield IS NULL AND year > 2010", "genre IN ('Comedy', 'Western', 'Fantasy')", "year < 1980",
         "rating > 5.5 AND rating < 8.5", "nosuchfield = 'x' OR genre = 'Drama'"]
BOOSTS = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low), Boost("rating > 8.0", BoostStrength.Med),
          Boost(None, BoostStrength.High), Boost("genre IN ('Action', 'Crime')", BoostStrength.Med)]
SORTS = [None, "year", "rating", "genre", "nosuchfield"]


@pytest.fixture(scope="module")
def fx():
    s = Synth(2, docs=40000)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    cols = columns(40000)
    year, rating, genre = cols
    for x in (e, o):
        x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
    qa, qo = s.queries(60, qseed=43, fuzz=0.3)
    return e, o, cols, Synth.texts(qa, qo), s


def mixed_queries(texts, n=120, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        t = texts[i % len(texts)]
        plain = rng.random() < 0.15
        if plain:                                                # no post-processing: any number of rows
            out.append(Query(t, int(rng.choice([10, 20, 100])), enable_coverage=bool(rng.random() < 0.7)))
            continue
        flt = None if rng.random() < 0.25 else EXPRS[int(rng.integers(len(EXPRS)))]
        nb = int(rng.integers(0, 4))
        boosts = [BOOSTS[j] for j in rng.choice(len(BOOSTS), nb, replace=False)] if nb else None
        out.append(Query(t, int(rng.choice([1, 5, 10, 20, 64])), enable_coverage=bool(rng.random() < 0.7), filter=flt,
                         enable_facets=bool(rng.random() < 0.5), enable_boost=boosts is not None and rng.random() < 0.8, boosts=boosts,
                         sort_by=SORTS[int(rng.integers(len(SORTS)))], sort_ascending=bool(rng.random() < 0.5)))
    return out


def alone(e, q):
    """The query on its own through the session-wide path (search_filtered installs its filter / boosts / sort for a batch of one)."""
    return e.search_filtered([q.text], q.max_number_of_records_to_return, q.coverage_depth, q.enable_coverage, q.filter, q.enable_facets,
                             enable_boost=q.enable_boost, boosts=q.boosts, sort_by=q.sort_by, sort_ascending=q.sort_ascending)[0]


def assert_same(r, w, ctx):
    assert r.error is None, (ctx, r.error)
    assert_rows(rows_of(r), rows_of(w), ctx)
    assert (r.unsupported, r.used_coverage, r.stage1_fallback, r.skipped_candidates) == (w.unsupported, w.used_coverage, w.stage1_fallback, w.skipped_candidates), ctx
    assert r.total_in_filter == w.total_in_filter, (ctx, r.total_in_filter, w.total_in_filter)
    assert (r.facets if r.facets is not None else None) == (w.facets if w.facets is not None else None), ctx


def test_mixed_batch_equals_each_query_alone(fx):
    e, o, cols, texts, _ = fx
    qs = mixed_queries(texts)
    res = e.search_queries(qs)
    assert len(res) == len(qs)
    checked = 0
    for q, r in zip(qs, res):
        w = alone(e, q)
        assert_same(r, w, (q.text, q.max_number_of_records_to_return, q.filter, q.sort_by))
        if q.max_number_of_records_to_return == 20 and q.enable_coverage and not (q.enable_boost and q.boosts) and q.sort_by is None:
            ow = o.search_filtered(q.text, 20, enable_coverage=True, filter=q.filter, enable_facets=q.enable_facets)
            assert [x.document_id for x in r.records] == ow["keys"], (q.text, q.filter)
            assert [x.tiebreaker for x in r.records] == ow["ties"].tolist(), (q.text, q.filter)
            assert r.total_in_filter == (ow["in_filter"] if q.filter is not None else 0)
            checked += 1
    assert any(len(r.records) > 64 for r in res)                 # rows beyond 64 for queries without post-processing, in the same batch
    assert checked > 0


def test_refused_queries_leave_their_neighbours_alone(fx):
    e, o, cols, texts, _ = fx
    qs = mixed_queries(texts, n=96, seed=11)
    bad = [Query(texts[0], 10, filter="year >= "), Query(texts[1], 10, filter="genre MATCHES '^D'"),
           Query(texts[2], 10, enable_boost=True, boosts=[Boost("year > %d" % y, BoostStrength.Low) for y in range(9)]),
           Query(texts[3], 100, enable_facets=True)]
    codes = [1, 5, 4, 5]                                         # INFX_EINVAL, INFX_EUNSUPPORTED, INFX_ECAPACITY, INFX_EUNSUPPORTED
    pos = [5, 30, 61, 90]
    mixed = list(qs)
    for p, b in zip(pos, bad):
        mixed.insert(p, b)
    res = e.search_queries(mixed)
    plain = e.search_queries(qs)
    others = [r for i, r in enumerate(res) if i not in pos]
    for q, r, w in zip(qs, others, plain):
        assert_same(r, w, q.text)
    for p in pos:
        assert res[p].records == [] and res[p].error, (p, res[p])
    # the raw flags and statuses of the same batch through the C ABI
    s = Session(e)
    status = _install_query_options(e, s.h, mixed)
    assert [int(status[p]) for p in pos] == codes
    assert all(int(x) == 0 for i, x in enumerate(status) if i not in pos)
    arena, offs = pack_texts([q.text for q in mixed])
    keys, scores, ties, counts, flags = s.search_packed(arena, offs, 100, 500, True)
    for p in pos:
        assert counts[p] == 0 and flags[p] & 16, (p, counts[p], flags[p])
    assert not any(flags[i] & 16 for i in range(len(mixed)) if i not in pos)


@pytest.mark.parametrize("k", [1, 2, 37, 300])
def test_first_use_counts_in_one_launch(fx, k):
    e, o, cols, texts, _ = fx
    exprs = ["year >= %d AND rating > %.2f AND genre != 'G%d'" % (1950 + j % 75, (j % 97) * 0.1, k) for j in range(k)]
    s = Session(e)
    qs = [Query(texts[j % len(texts)], 10, filter=x) for j, x in enumerate(exprs)]
    res = s.search_queries(qs)
    assert s.last_count_stats() == (k, 1)
    for x, r in zip(exprs, res):                                 # every program of the launch (past 256: a second round of the LDS counters' stride)
        assert r.total_in_filter == o.search_filtered(texts[0], 10, filter=x)["in_filter"], x
    again = s.search_queries(qs)                                 # cached: nothing counted
    assert s.last_count_stats() == (0, 0)
    assert [r.total_in_filter for r in again] == [r.total_in_filter for r in res]
    t = Session(e)
    for x, r in zip(exprs[:8], res[:8]):
        assert t.set_filter(x) == r.total_in_filter              # the session-wide path reports the cached number
    t.set_filter(None)


def test_session_count_on_a_fresh_cache_equals_the_batched_count(fx):
    """infx_filter_count (the session-wide path, one program per launch) on an engine whose cache has never seen the expressions, against the
    batched count of the same expressions on the fixture's engine (programs 0..299 of one launch) and the oracle."""
    e, o, cols, texts, s = fx
    exprs = ["rating <= %.1f OR genre IN ('Western', 'F%d')" % (1.0 + (j % 90) * 0.1, j) for j in range(300)]
    res = Session(e).search_queries([Query(texts[j % len(texts)], 10, filter=x) for j, x in enumerate(exprs)])
    arena, offs = s.docs()
    f = SearchEngine.create_default(device=0); f.index_flat(None, arena, offs, s.field_weights)
    year, rating, genre = cols
    f.set_column("year", year, facetable=True); f.set_column("rating", rating, facetable=False); f.set_column("genre", genre, facetable=True)
    t = Session(f)
    for j in list(range(0, 300, 37)) + [255, 256, 257, 299]:
        n = t.set_filter(exprs[j])
        assert n == res[j].total_in_filter == o.search_filtered(texts[0], 10, filter=exprs[j])["in_filter"], exprs[j]
    t.set_filter(None)


def test_host_phases_refuse_post_processing(tmp_path):
    """INFX_PHASED=1 (host phases, no device finalize): a query with a filter, facets, boosts or sort is refused on its own (INFX_EUNSUPPORTED,
    empty, flag bit 4) instead of coming back unfiltered; the per-query row count and coverage still apply to the others."""
    import os
    import subprocess
    import sys
    script = r'''
import sys
import numpy as np
from infidex_amd import SearchEngine, Query, Boost
from infidex_amd.engine import Session, pack_texts, _install_query_options
from tools.synth import Synth
s = Synth(2, docs=20000); arena, offs = s.docs()
e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
e.set_column("year", np.arange(20000, dtype=np.int64) % 75 + 1950, facetable=True)
qa, qo = s.queries(8, qseed=5, fuzz=0.3); tx = Synth.texts(qa, qo)
qs = [Query(tx[0], 7), Query(tx[1], 10, filter="year > 2000"), Query(tx[2], 10, enable_facets=True), Query(tx[3], 3, enable_coverage=False),
      Query(tx[4], 10, enable_boost=True, boosts=[Boost("year > 2000", 2)]), Query(tx[5], 10, sort_by="year")]
se = Session(e)
st = _install_query_options(e, se.h, qs)
assert st.tolist() == [0, 5, 5, 0, 5, 5], st
k, sc, t, c, f = se.search_packed(*pack_texts([q.text for q in qs]), 10, 500, True)
assert [int(c[i]) for i in (1, 2, 4, 5)] == [0, 0, 0, 0] and all(f[i] & 16 for i in (1, 2, 4, 5)), (c, f)
assert not (f[0] & 16) and not (f[3] & 16) and 0 < c[0] <= 7 and 0 < c[3] <= 3, (c, f)
plain = e.search_batch([tx[0], tx[3]], 10, enable_coverage=True)
assert k[0, :int(c[0])].tolist() == [x.document_id for x in plain[0].records][:7]
alone = e.search_batch([tx[3]], 3, enable_coverage=False)[0]
assert k[3, :int(c[3])].tolist() == [x.document_id for x in alone.records]
r = se.search_queries(qs)
assert [x.error is not None for x in r] == [False, True, True, False, True, True]
'''
    env = dict(os.environ); env["INFX_PHASED"] = "1"
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", script], check=True, env=env, timeout=600)


def test_evicted_expressions_count_again(fx):
    e, o, cols, texts, _ = fx
    exprs = ["year <= %d OR genre = 'E%d'" % (1960 + j, j) for j in range(30)]
    s = Session(e)
    qs = [Query(texts[j % len(texts)], 10, filter=x) for j, x in enumerate(exprs)]
    first = [r.total_in_filter for r in s.search_queries(qs)]
    e.set_filter_cache_limit(8)
    try:
        assert e.filter_cache_size() <= 8
        res = s.search_queries(qs[:5])
        assert s.last_count_stats()[0] == 5                      # evicted: counted again
        assert [r.total_in_filter for r in res] == first[:5]
    finally:
        e.set_filter_cache_limit(4096)


def test_counts_follow_deletions():
    docs = [Document(k, "alpha bravo %d" % k) for k in range(1, 9)]
    year = np.array([1990, 1995, 2000, 2005, 2010, 2015, 2020, 2025], np.int64)
    e = SearchEngine.create_default(device=0); e.index_documents(docs); e.set_column("year", year, facetable=True)
    o = O.OracleEngine.create_default(); o.index([(d.document_key, d.fields) for d in docs]); o.set_column("year", year, facetable=True)
    for step in range(2):
        r = e.search_queries([Query("alpha", 10, filter="year >= 2000"), Query("alpha", 10)])
        w = o.search_filtered("alpha", 10, filter="year >= 2000")
        assert r[0].total_in_filter == w["in_filter"] == (6 if step == 0 else 4)
        assert [x.document_id for x in r[0].records] == w["keys"]
        assert r[1].total_in_filter == 0
        e.delete_documents([3, 8]); o.delete_keys([3, 8])
    e.restore_documents()
    assert e.search_queries([Query("alpha", 10, filter="year >= 2000")])[0].total_in_filter == 6


def test_three_shards_equal_unsharded(fx):
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_search_queries
    e, o, cols, texts, s = fx
    arena, offs = s.docs()
    year, rating, genre = cols
    W = 3
    engs = [create_sharded_engine(r, W, 0) for r in range(W)]
    for x in engs:
        x.index_flat(None, arena, offs, s.field_weights)
        x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
    sess = [ShardSession(x) for x in engs]
    qs = mixed_queries(texts, n=96, seed=5)
    got = simulate_search_queries(sess, qs, every_shard=True)
    want = e.search_queries(qs)
    assert len(got) == W
    for shard, rows in enumerate(got):                            # every shard: the same rows, facets and GLOBAL counts
        for q, r, w in zip(qs, rows, want):
            assert_same(r, w, (shard, q.text))


def test_contract(fx):
    e, o, cols, texts, _ = fx
    s = Session(e)
    s.set_filter("year > 2000")
    with pytest.raises(InfidexError) as ei:
        s.search_queries([Query(texts[0], 10, filter="year < 1990")])
    assert ei.value.code == 1
    s.set_filter(None)
    _install_query_options(e, s.h, [Query(texts[0], 10, filter="year < 1990")])
    with pytest.raises(InfidexError) as ei:
        s.set_filter("year > 2000")
    assert ei.value.code == 1
    with pytest.raises(InfidexError) as ei:                      # nq mismatch: refused, and the options are gone
        s.search_packed(*pack_texts(texts[:2]), 10, 500, True)
    assert ei.value.code == 1
    s.search_queries([Query(texts[0], 10, filter="year < 1990", sort_by="year")])
    nxt = s.search_packed(*pack_texts(texts[:1]), 10, 500, True)          # the next batch is plain
    plain = e.search_batch(texts[:1], 10)[0]
    assert [int(k) for k in nxt[0][0, :int(nxt[3][0])]] == [x.document_id for x in plain.records]
