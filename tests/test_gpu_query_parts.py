"""The four per-query parts of a batch (options, coverage setups, pre-filters, collapse requests) together on the GPU: each refuses a query of one batch on
its own, a query two parts refuse reports the earlier part's message, the accepted queries answer as in a batch of their own, nothing outlives the batch;
and a sharded batch abandoned after its phase 0 leaves nothing behind for the next one."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, CoverageSetup
from infidex_amd.engine import Session, pack_texts
from tests.test_gpu_collapse import small_engine, same_answer

pytestmark = pytest.mark.gpu

BAD_SETUP = CoverageSetup(truncation_score=999)


def test_all_four_parts_refuse_in_one_batch():
    e, _ = small_engine(300)
    good = [Query("alpha", 10, collapse_by="ten", collapse_keep=2), Query("alpha lot 7", 5), Query("red alpha", 10, filter="year >= 1980"),
            Query("golden", 20, pre_filter="year >= 1970", coverage_setup=CoverageSetup(truncate=False)), Query("green lot 12", 10, collapse_by="word")]
    bad = {1: (Query("alpha", 10, filter="year >= "), "syntax"),                                         # options
           3: (Query("alpha", 10, coverage_setup=BAD_SETUP), "TruncationScore"),                         # coverage
           4: (Query("golden", 10, pre_filter="genre MATCHES '^D'"), "MATCHES"),                         # pre-filter
           6: (Query("alpha", 10, collapse_by="nosuch"), "nosuch"),                                      # collapse
           8: (Query("red", 10, coverage_setup=BAD_SETUP, collapse_by="nosuch"), "TruncationScore")}     # coverage and collapse: coverage comes first
    mix = list(good)
    for p in sorted(bad):
        mix.insert(p, bad[p][0])
    assert len(mix) == 10
    s = Session(e)
    try:
        res = s.search_queries(mix)
        for p, (_, word) in bad.items():
            assert res[p].records == [] and res[p].error and word in res[p].error, (p, res[p])
        assert "nosuch" not in res[8].error
        alone = Session(e)
        try:
            want = alone.search_queries(good)
        finally:
            alone.close()
        for i, (r, w) in enumerate(zip([r for p, r in enumerate(res) if p not in bad], want)):
            assert r.error is None
            same_answer(r, w, ("accepted", i))
        # nothing leaked: a plain batch of the same size on the same session
        texts = [q.text for q in mix]
        keys, scores, ties, counts, flags = s.search_packed(*pack_texts(texts), 10, 500, True)
        plain = e.search_batch(texts, 10)
        for i, w in enumerate(plain):
            n = int(counts[i])
            assert [int(k) for k in keys[i, :n]] == [x.document_id for x in w.records], texts[i]
            assert np.array_equal(scores[i, :n].view(np.uint32), np.asarray([x.score for x in w.records], np.float32).view(np.uint32)), texts[i]
            assert not int(flags[i]) & 16
        assert s.last_collapse_stats() == (0, 0)
    finally:
        s.close()


def test_an_abandoned_sharded_batch_leaves_nothing_behind():
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards_dev
    docs = [Document(k, "alpha bravo %d" % k) for k in range(40)]
    engs = [create_sharded_engine(r, 2, 0) for r in range(2)]
    for x in engs:
        x.index_documents(docs)
    sess = [ShardSession(x) for x in engs]
    qs = [Query("alpha", 10), Query("bravo 7", 5, coverage_setup=CoverageSetup(truncate=False))]
    arena, offs = pack_texts([q.text for q in qs])
    for s in sess:
        assert s.set_query_options(qs).tolist() == [0, 0]
        s.phase0(arena, offs, 500)                       # the options and the setups are bound to this batch, which goes no further
    plain = pack_texts(["alpha", "bravo 7", "alpha bravo 31"])
    got = simulate_shards_dev(sess, *plain, 10)
    want = simulate_shards_dev([ShardSession(x) for x in engs], *plain, 10)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert np.array_equal(a, b)
    assert int(got[0][3].sum()) > 0
