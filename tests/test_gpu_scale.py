"""GPU parity at a larger scale (BASELINE config 4 shape, 400k docs) and size-independent properties of the device pipeline.

Against the oracle: a 120-query sample (the oracle needs ~30 ms per query at this size).  Exact BM25 ties at the Stage-1 top-500
cut-off are resolved by the reference through BCL heap order (unpinned), so a small fraction of queries may
differ in their final sets; every other query must match exactly.
Properties (no oracle needed, any size): ordering of the returned rows, determinism, independence from batching, equality of the
packed and unpacked posting layouts, equality of the document-sharded and the single-index pipelines.
"""
import os

import numpy as np
import pytest

from infidex_amd import SearchEngine
from infidex_amd.engine import pack_texts
from tests import oracle_lib as O
from tools.synth import Synth

pytestmark = pytest.mark.gpu

N_DOCS = 400_000
K = 20


@pytest.fixture(scope="module")
def corpus():
    s = Synth(4, docs=N_DOCS)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, s.field_weights)
    qa, qo = s.queries(1000, qseed=4242)
    return s, arena, offs, e, Synth.texts(qa, qo)


@pytest.fixture(scope="module")
def oracle(corpus):
    s, arena, offs, e, texts = corpus
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    return o


def run(e, texts, k=K):
    a, o = pack_texts(texts)
    return e.search_packed(a, o, k)


def test_rows_are_ordered_and_unique(corpus):
    _, _, _, e, texts = corpus
    keys, scores, ties, counts, flags = run(e, texts)
    assert counts.max() <= K and counts.sum() > 0
    for i in range(len(texts)):
        c = int(counts[i])
        ks = keys[i, :c].tolist()
        assert len(set(ks)) == c                                         # ConsolidateSegments: one row per DocumentKey
        rows = [(-float(scores[i, j]), -int(ties[i, j]), int(keys[i, j])) for j in range(c)]
        if flags[i] & 2 and not flags[i] & 4:                            # coverage rows: ScoreEntry order (score desc, tie desc, key asc)
            assert rows == sorted(rows), (texts[i], rows)
        else:                                                            # Stage-1 rows: score desc, key asc
            r1 = [(-float(scores[i, j]), int(keys[i, j])) for j in range(c)]
            assert r1 == sorted(r1), (texts[i], r1)


def test_deterministic_and_batch_independent(corpus):
    _, _, _, e, texts = corpus
    a = run(e, texts)
    b = run(e, texts)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                                      # idempotent: same batch, same bits
    sub = list(range(0, len(texts), 37))
    c = run(e, [texts[i] for i in sub])
    for j, i in enumerate(sub):
        n = int(a[3][i])
        assert int(c[3][j]) == n
        assert np.array_equal(c[0][j, :n], a[0][i, :n]) and np.array_equal(c[1][j, :n], a[1][i, :n]) and np.array_equal(c[2][j, :n], a[2][i, :n])


def test_unpacked_layout_equals_packed(corpus):
    s, arena, offs, e, texts = corpus
    os.environ["INFX_UNPACKED"] = "1"                                    # read when the postings are uploaded
    try:
        u = SearchEngine.create_default(device=0)
        u.index_flat(None, arena, offs, s.field_weights)
    finally:
        del os.environ["INFX_UNPACKED"]
    a = run(e, texts[:400]); b = run(u, texts[:400])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_sharded_equals_the_oracle_at_scale(corpus, oracle):
    """Four doc-range shards of the 400k-doc corpus (7 containers: 1 + 2 + 2 + 2) through the RCCL code path (device exchange tensors) against the ORACLE:
    no query may differ — the exact Stage-1 replay runs across the shards (first-pass lists, global ambiguity test, per-shard chunks, owner-side heap)."""
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards_dev
    from tests.parity_classify import assert_final_rows_match_oracle
    s, arena, offs, e, texts = corpus
    W = 4
    engs = [create_sharded_engine(r, W, 0) for r in range(W)]
    for g in engs:
        g.index_flat(None, arena, offs, s.field_weights)
    assert all(g.shard_info()[0] % 65536 == 0 and g.shard_info()[1] > 0 for g in engs)
    sess = [ShardSession(g) for g in engs]
    a2, o2 = pack_texts(texts[:500])
    res = simulate_shards_dev(sess, a2, o2, K)
    for r in res[1:]:
        for x, y in zip(r, res[0]):
            assert np.array_equal(x, y)
    keys, scores, ties, counts, flags = res[0]
    sample = list(range(0, 500, 3))
    same, flips, inexact = assert_final_rows_match_oracle(keys[sample], scores[sample], counts[sample], oracle, [texts[i] for i in sample], K, what="4 shards at 400k docs")
    replays = sum(x.s.last_timings()["exact_replays"] for x in sess)
    print("4 shards vs oracle:", same, "identical order,", flips, "near-tie flips of", len(sample), ",", inexact, "rows not bit-equal; queries replayed on their owners:", replays)
    assert replays > 0
    # and the single index returns the same sets for the whole batch (both are the reference's)
    ref = e.search_packed(a2, o2, K)
    assert np.array_equal(ref[3], counts)
    for i in range(500):
        assert set(ref[0][i, :int(counts[i])].tolist()) == set(keys[i, :int(counts[i])].tolist()), texts[i]


def test_oracle_sample_at_scale(corpus, oracle):
    """Final top-k sets AND order vs the oracle at 400k docs.  With the exact Stage-1 replay (k_exact1) no query may differ; should one
    differ it is classified (tests/parity_classify.py) and anything that is not a cut-off tie fails with its dump."""
    from tests.parity_classify import classify, assert_final_rows, stage2_scored
    s, arena, offs, e, texts = corpus
    o = oracle
    sample = texts[:160]
    keys, scores, ties, counts, flags = run(e, sample)
    differ, order_differ, inexact = [], 0, 0
    for i, q in enumerate(sample):
        r = o.search(q, K, 500)
        got = keys[i, :int(counts[i])].tolist()
        if set(got) != set(r["keys"]):
            differ.append(q)
            continue
        # the oracle's score bits or one ulp off; order flips only between one-ulp near-ties with a row that is not bit-equal
        bad, swaps = assert_final_rows(got, scores[i, :len(got)], r["keys"], r["scores"], stage2_scored(o, r), q)
        inexact += bad
        order_differ += got != r["keys"]
    cls = classify(e, o, differ, K) if differ else []
    print("scale sample:", len(sample) - len(differ), "identical,", order_differ, "order flips,", inexact, "rows not bit-equal,", cls)
    assert not [c for c in cls if c["kind"] == "other"], cls
    assert len(differ) == 0, cls            # exact replay: no cut-off tie may survive either
    t = e.last_timings()
    print("exact replays in the last batch:", t["exact_replays"])


def test_exact_replay_off_keeps_doc_order_ties(corpus):
    """exact_replay=False (INFX_CFG_NO_EXACT_REPLAY, a measurement switch — no product path runs without the replay): the cut is taken by (score, doc id);
    still deterministic and within the tie rule."""
    s, arena, offs, e, texts = corpus
    u = SearchEngine.create_default(device=0, exact_replay=False)
    u.index_flat(None, arena, offs, s.field_weights)
    a = run(u, texts[:300]); b = run(u, texts[:300])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert u.last_timings()["exact_replays"] == 0
    c = run(e, texts[:300])
    same = sum(1 for i in range(300) if set(a[0][i, :int(a[3][i])].tolist()) == set(c[0][i, :int(c[3][i])].tolist()))
    print("exact vs doc-order cut: identical final sets", same, "/ 300; exact replays", e.last_timings()["exact_replays"])
    assert same >= 285


def test_deleted_documents_at_scale(corpus, oracle):
    """Deletions at 400k documents, through the exact Stage-1 replay: a deleted document keeps its position in the reference's chunks and match
    lists (so the Vector256 / scalar-tail split of its neighbours is unchanged) but never reaches the heap.  Oracle sample must be identical;
    the document-sharded pipeline with the same deletions must give the oracle's rows as well."""
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards_dev
    s, arena, offs, e, texts = corpus
    rng = np.random.default_rng(77)
    sample = texts[160:280]
    keys0, _, _, counts0, _ = run(e, sample)
    gone = set(rng.choice(N_DOCS, N_DOCS // 10, replace=False).tolist())
    for i in range(len(sample)):
        gone.update(keys0[i, :min(3, int(counts0[i]))].tolist())                    # and the best rows of every sampled query
    gone = np.asarray(sorted(gone), np.int64)
    o = oracle
    try:
        assert e.delete_documents(gone) == len(gone) and o.delete_keys(gone) == len(gone)
        keys, scores, ties, counts, flags = run(e, sample)
        replays = e.last_timings()["exact_replays"]
        gs = set(gone.tolist()); differ = 0
        for i, q in enumerate(sample):
            got = keys[i, :int(counts[i])].tolist()
            assert not (set(got) & gs), q
            r = o.search(q, K, 500)
            if set(got) != set(r["keys"]):
                differ += 1; print("differs:", q, got, r["keys"])
        print("deleted sample:", len(sample) - differ, "identical of", len(sample), "; exact replays", replays)
        assert differ == 0
        # shards: same deletions on every rank; the cross-shard replay must give the oracle's rows too
        from tests.parity_classify import assert_final_rows_match_oracle
        W = 2
        engs = [create_sharded_engine(r, W, 0) for r in range(W)]
        for g in engs:
            g.index_flat(None, arena, offs, s.field_weights); g.delete_documents(gone)
        a2, o2 = pack_texts(sample)
        res = simulate_shards_dev([ShardSession(g) for g in engs], a2, o2, K)
        for x, y in zip(res[0], res[1]):
            assert np.array_equal(x, y)
        assert_final_rows_match_oracle(res[0][0], res[0][1], res[0][3], o, sample, K, what="2 shards with deletions")
    finally:
        e.restore_documents()
        o.restore_all()


def test_host_phase_implementation_equals_device_pipeline(tmp_path):
    """INFX_PHASED=1 routes a single-GPU engine through the stage-wise C ABI (infx_stage1_accumulate / _select, infx_stage2_batch) with the
    host implementation of tier rules, candidate assembly and final ordering.  It must agree bit for bit with the device pipeline."""
    import subprocess
    import sys
    script = r'''
import sys, numpy as np
from infidex_amd import SearchEngine
from infidex_amd.engine import pack_texts
from tools.synth import Synth
s = Synth(2, docs=20000); arena, offs = s.docs()
e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
qa, qo = s.queries(300, qseed=9, fuzz=0.3)
tx = Synth.texts(qa, qo)
longq = " ".join(dict.fromkeys(w for t in tx[:40] for w in t.split()))      # > 32 distinct words: the long-query launches, in both implementations
assert len(longq.split()) > 32
a, o = pack_texts(tx + ["qu", "", "zzzzqq", longq, "x" * 600])
k, sc, t, c, f = e.search_packed(a, o, 10)
# an over-long document (260 words: third k_stage2 launch) is ranked like any other; a query beyond the long envelope (INFX_LONGQ_CHARS) is answered as unsupported (flag bit 0)
from infidex_amd import Document
e2 = SearchEngine.create_default(device=0)
e2.index_documents([Document(0, " ".join("word%d" % i for i in range(260))), Document(1, "word0 word1"), Document(2, "charlie delta"), Document(3, "word0 word1 charlie")])
a2, o2 = pack_texts(["word0 word1", "charlie delta", "x" * 2100])
k2, sc2, t2, c2, f2 = e2.search_packed(a2, o2, 5)
assert not (f2[0] & 8) and 0 in k2[0, :int(c2[0])].tolist() and not (f2[1] & 8) and f2[2] & 1 and c2[2] == 0, (f2, k2)
np.savez(sys.argv[1], k=k, sc=sc, t=t, c=c, f=f, k2=k2, sc2=sc2, c2=c2, f2=f2)
'''
    outs = []
    for phased in ("0", "1"):
        env = dict(os.environ); env.pop("INFX_PHASED", None)
        if phased == "1":
            env["INFX_PHASED"] = "1"
        env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        path = str(tmp_path / f"r{phased}.npz")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=env, timeout=600)
        outs.append(np.load(path))
    a, b = outs
    assert np.array_equal(a["c"], b["c"]) and np.array_equal(a["f"], b["f"])
    assert np.array_equal(a["c2"], b["c2"]) and np.array_equal(a["f2"], b["f2"])
    for i in range(3):
        n = int(a["c2"][i]); assert np.array_equal(a["k2"][i, :n], b["k2"][i, :n]) and np.array_equal(a["sc2"][i, :n], b["sc2"][i, :n])
    for i in range(len(a["c"])):
        n = int(a["c"][i])
        assert np.array_equal(a["k"][i, :n], b["k"][i, :n]) and np.array_equal(a["sc"][i, :n], b["sc"][i, :n]) and np.array_equal(a["t"][i, :n], b["t"][i, :n])


def test_concurrent_sessions_match_sequential_results(corpus):
    """ThreadSafetyTests.cs:16-43,139-175 (many readers under the read lock): several host threads, one engine session each, searching the
    same index at once return exactly what a sequential caller gets."""
    import threading
    from infidex_amd import Session
    _, _, _, e, texts = corpus
    batches = [texts[i:i + 100] for i in range(0, 800, 100)]
    expect = [run(e, b) for b in batches]
    sessions = [Session(e) for _ in range(4)]
    got = [None] * len(batches); errors = []

    def worker(w):
        try:
            for rep in range(3):
                for bi in range(w, len(batches), 4):
                    a, o = pack_texts(batches[bi])
                    got[bi] = sessions[w].search_packed(a, o, K)
        except Exception as ex:   # surfaced below
            errors.append(ex)
    ths = [threading.Thread(target=worker, args=(w,)) for w in range(4)]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errors, errors
    for g, x in zip(got, expect):
        for u, v in zip(g, x):
            assert np.array_equal(u, v)


def test_parallel_exact_replay_equals_the_sequential_kernel(tmp_path):
    """The production replay (k_ex_scan / k_ex_chunk / k_ex_heap) and the literal sequential kernel (k_exact1, INFX_EXACT_SLOW=1) are two
    implementations of the same reference semantics: final rows AND the Stage-1 rows (sets, fp32 score bits) must be identical."""
    import subprocess
    import sys
    script = r'''
import sys, numpy as np
from infidex_amd import SearchEngine
from infidex_amd.engine import pack_texts
from tools.synth import Synth
s = Synth(4, docs=300000); arena, offs = s.docs()
e = SearchEngine.create_default(device=0, want_features=True); e.index_flat(None, arena, offs, s.field_weights)
qa, qo = s.queries(400, qseed=77)
texts = Synth.texts(qa, qo)
a, o = pack_texts(texts)
k, sc, t, c, f = e.search_packed(a, o, 20)
s1k = []; s1s = []
for i in range(len(texts)):
    kk, ss = e.last_stage1(i)
    s1k.append(np.asarray(kk, np.int64)); s1s.append(np.asarray(ss, np.float32))
n = e.last_timings()["exact_replays"]
np.savez(sys.argv[1], k=k, sc=sc, t=t, c=c, f=f, s1k=np.concatenate(s1k), s1s=np.concatenate(s1s), s1n=np.asarray([len(x) for x in s1k]), replays=n)
'''
    outs = []
    for slow in ("0", "1"):
        env = dict(os.environ); env.pop("INFX_EXACT_SLOW", None)
        if slow == "1":
            env["INFX_EXACT_SLOW"] = "1"
        env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        path = str(tmp_path / f"x{slow}.npz")
        subprocess.run([sys.executable, "-c", script, path], check=True, env=env, timeout=900)
        outs.append(np.load(path))
    a, b = outs
    print("exact replays:", int(a["replays"]), int(b["replays"]))
    assert int(a["replays"]) > 20 and int(a["replays"]) == int(b["replays"])
    for key in ("k", "sc", "t", "c", "f", "s1n", "s1k"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["s1s"].view(np.uint32), b["s1s"].view(np.uint32))
