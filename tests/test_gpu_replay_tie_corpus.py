"""The tie corpus of tests/test_replay_model.py (replay_model.tie_corpus: 140 000 short documents from 40 templates, thousands of them equal in length and in every
matched term; queries at depths 1, 7, 64 and 500) on the whole engine against the oracle: unsharded, the Stage-1 sets and score bits; on three simulated shards
(container-aligned: the shard boundaries cut the plateaus), the final rows, with the cross-shard replay (k_gflag, k_exsh_*, the owner-side heap) having run."""
import numpy as np
import pytest

from tests import oracle_lib as O
from tests import replay_model as RM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tie():
    from infidex_amd.engine import pack_texts
    texts, queries = RM.tie_corpus()
    arena, offs = pack_texts(texts)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs); o.finalize()
    by_depth = {d: [q for q, k in queries if k == d] for d in RM.TIE_DEPTHS}
    return arena, offs, o, by_depth


def test_unsharded_stage1_rows_are_the_oracles_bit_for_bit(tie):
    from infidex_amd import SearchEngine
    arena, offs, o, by_depth = tie
    e = SearchEngine.create_default(device=0, want_features=True); e.index_flat(None, arena, offs)      # want_features: the engine keeps the Stage-1 rows for last_stage1
    replays = rows = 0
    for depth, qs in by_depth.items():
        e.search_batch(qs, 10, depth)
        replays += e.last_timings()["exact_replays"]
        for i, q in enumerate(qs):
            o.search(q, 10, depth)
            ok, osc = o.last_stage1()
            gk, gs = e.last_stage1(i)
            want = dict(zip(ok.tolist(), osc.view(np.uint32).tolist())); got = dict(zip(gk.tolist(), gs.view(np.uint32).tolist()))
            assert len(gk) == len(ok) == len(got), (q, depth, len(gk), len(ok))
            assert set(got) == set(want), (q, depth, "documents", sorted(set(got) ^ set(want))[:10])
            wrong = [(d, hex(got[d]), hex(want[d])) for d in want if got[d] != want[d]]
            assert not wrong, (q, depth, "score bits", len(wrong), wrong[:5])
            rows += len(ok)
    print(f"tie corpus, unsharded: {sum(len(v) for v in by_depth.values())} queries, {rows} Stage-1 rows bit-equal to the oracle's, {replays} queries replayed exactly")
    assert replays > 0


def test_three_shards_equal_the_oracle(tie):
    from infidex_amd.engine import pack_texts
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards
    from tests.parity_classify import assert_final_rows_match_oracle
    arena, offs, o, by_depth = tie
    W = 3
    for depth, qs in by_depth.items():                     # document shards search with CoverageDepth == the engine's max_depth: one set of engines per depth
        engs = [create_sharded_engine(r, W, 0, max_depth=depth) for r in range(W)]
        for e in engs:
            e.index_flat(None, arena, offs)
        assert [b for b, _ in (e.shard_info() for e in engs)] == [0, 65536, 131072]
        sess = [ShardSession(e) for e in engs]
        a2, o2 = pack_texts(qs)
        k, sc, t, c, f = simulate_shards(sess, a2, o2, 10, depth)[0]
        same, flips, inexact = assert_final_rows_match_oracle(k, sc, c, o, qs, 10, depth=depth, what=f"tie corpus, 3 shards, depth {depth}")
        replays = sum(x.s.last_timings()["exact_replays"] for x in sess)
        print(f"tie corpus, 3 shards, depth {depth}: {same} identical order, {flips} near-tie flips, {inexact} rows not bit-equal; replayed on their owners: {replays}")
        assert replays > 0, depth
        del sess, engs
