"""GPU parity: the HIP path (through the C ABI) vs the oracle on the same inputs.  Run with `-m gpu` on an MI355X.

Bars (north star): DocumentId sets of the final top-k bit-exact, Stage-2 features (integer counts and float features) bit-exact, Stage-2
scores bit-exact wherever the Stage-1 base agrees, within one ulp plus the moved BM25 share where it does not (compare_batch).  Stage-1 BM25 scores: the reference itself mixes two arithmetically different formulas depending on
a document's position in a chunk (quirk Q9, Bm25Scorer.cs:395-444); the device uses the 8-lane formula throughout, so
Stage-1 scores agree to SCORE_RTOL and top-`depth` sets may differ only among documents whose oracle scores are within
that tolerance of the cut-off.
"""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document
from tests import oracle_lib as O
from tests.test_oracle_kats import TEN_DOCS, BATMAN20, DARK20
from tests.parity_classify import SCORE_RTOL, bits, blend_slack, score_matches, assert_final_rows, stage2_scored
from tools.synth import Synth

pytestmark = pytest.mark.gpu

N_CMP_FEAT = 31             # feat[0, 25): integer counts; feat[25, 31): SumCi, IdfCoverage, TotalIdf, MissingIdf, LastTermCi, WeightedCoverage as fp32 bits


def gpu_engine(**kw):
    return SearchEngine.create_default(device=0, want_features=True, **kw)


@pytest.fixture(scope="module")
def ten():
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in TEN_DOCS])
    o = O.OracleEngine.create_default(); o.index(TEN_DOCS)
    return e, o


def test_reference_kats_on_gpu(ten):
    e, _ = ten
    # ReferenceMatchingTests.cs:39-98 (exact lists)
    r = e.search_batch(["batman", "qick fux", "battamam", "new york", "speeding"], 10)
    ids = [[x.document_id for x in rr.records] for rr in r]
    assert ids[0][0] == 6
    assert ids[1] == [5, 1]
    assert ids[2] == [6]
    assert ids[3] == [8]
    assert ids[4] == [7]


def test_more_reference_kats_on_gpu():
    e = gpu_engine(); e.index_documents([Document(i, "batman saves the day") for i in range(20)])
    assert len(e.search("batman", 5).records) == 5                                   # QueryTests.cs:150-169
    e = gpu_engine(); e.index_documents([Document(i, f"batman saves the day story {i}") for i in range(20)])
    assert len(e.search("batman", 8).records) == 8                                   # :171-189
    e = gpu_engine(); e.index_documents([Document(i, t) for i, t in enumerate(BATMAN20)])
    assert len(e.search("batman", 12).records) == 12                                 # :191-225
    e = gpu_engine(); e.index_documents([Document(i, t) for i, t in enumerate(DARK20)])
    r = e.search("dark knight rises", 10).records                                    # :227-277
    assert r[0].document_id == 5 and 8 in [x.document_id for x in r[:3]]
    assert all(r[i - 1].score >= r[i].score for i in range(1, len(r)))
    e = gpu_engine(); e.index_documents([Document(1, "hello world"), Document(2, "goodbye world"), Document(3, "hello there")])
    r = e.search("hello world", 10).records                                          # SearchEngineTests.cs:37-54
    assert r[0].document_id == 1 and r[0].score > 200
    e = SearchEngine.create_minimal(device=0); e.index_documents([Document(1, "hello world"), Document(2, "goodbye world")])
    r = e.search("hello", 10)                                                        # :150-164
    assert r.records[0].document_id == 1 and not r.used_coverage
    assert e.search("", 10).records == []                                            # :77-90


def compare_batch(e, o, queries, k, depth=500, check_features=True):
    """Runs `queries` through the GPU engine (one batch) and the oracle (one by one); returns mismatch statistics.

    Stage 2, per evaluated (document, base) row: features feat[:31] (the integer counts and the six float features as bits) and the tiebreaker bit-exact;
    the base score bit-exact on every row of a query whose Stage-1 rows are bit-exact; the score bit-exact where the base bits agree or the row's coverage is
    not partial (the base enters FusionScorer only through `partial && bm25 >= gap`), else within one ulp plus what the base difference moves the BM25 share
    (parity_classify.score_matches / blend_slack).  Final rows: parity_classify.assert_final_rows."""
    o.set_trace(True)
    res = e.search_batch(queries, k, depth)
    qo, docs, base, sc, ties, feat = e.last_stage2()
    # group device Stage-2 records per cov-query index in order
    order = {}
    for i in range(len(qo)):
        order.setdefault(int(qo[i]), []).append(i)
    cov_idx = 0
    stats = dict(n=0, set_mismatch=0, order_mismatch=0, feat_mismatch=0, s1_boundary=0, s1_bitexact=0, max_s1_rel=0.0, s2_rows=0, base_mismatch=0,
                 s2_inexact=0, final_inexact=0, max_final_abs=0.0)
    for qi, q in enumerate(queries):
        r = o.search(q, k, depth)
        got = res[qi]
        stats["n"] += 1
        # ---- Stage 1: scores and sets
        ok, osc = o.last_stage1()
        gk, gsc = e.last_stage1(qi)
        od = dict(zip(ok.tolist(), osc.tolist()))
        gd = dict(zip(gk.tolist(), gsc.tolist()))
        for key in set(od) & set(gd):
            rel = abs(od[key] - gd[key]) / max(abs(od[key]), 1e-9)
            stats["max_s1_rel"] = max(stats["max_s1_rel"], rel)
            assert rel <= SCORE_RTOL, (q, key, od[key], gd[key])
        s1_exact = set(od) == set(gd) and all(bits(od[key]) == bits(gd[key]) for key in od)
        if s1_exact:
            stats["s1_bitexact"] += 1
        if set(od) != set(gd):
            # allowed only at the cut-off: every doc in the symmetric difference scores within tolerance of the k-th score
            cut = min(osc) if len(osc) else 0.0
            for key in set(od) ^ set(gd):
                s = od.get(key, gd.get(key))
                assert abs(s - cut) <= SCORE_RTOL * max(abs(cut), 1.0) * 4, (q, key, s, cut)
            stats["s1_boundary"] += 1
        # ---- Stage 2: features, base, tie and score per evaluated (doc, base) pair, in the oracle's evaluation order
        if got.used_coverage:
            assert r["used_coverage"], q
            idxs = order.get(cov_idx, []); cov_idx += 1
            tids, tbase, tsc, tties, tfeat = o.last_trace()
            if check_features and set(od) == set(gd):
                assert len(idxs) == len(tids), (q, len(idxs), len(tids))
                # same evaluations; the order inside the TF-IDF section may differ between documents whose Stage-1 scores differ by less than SCORE_RTOL
                # (quirk Q9), so pair records by document: a document evaluated twice (WordMatcher overlap row with base 0, then its Stage-1 row) pairs by
                # its base bits where they agree, else by occurrence number
                assert sorted(docs[idxs].tolist()) == sorted(tids.tolist()), q
                slots = {}
                for a, d in enumerate(tids.tolist()):
                    slots.setdefault(d, []).append(a)
                for i in idxs:
                    free = slots[int(docs[i])]
                    a = next((x for x in free if bits(tbase[x]) == bits(base[i])), free[0]); free.remove(a)
                    stats["s2_rows"] += 1
                    if not np.array_equal(feat[i, :N_CMP_FEAT], tfeat[a, :N_CMP_FEAT]):
                        stats["feat_mismatch"] += 1
                        bad = [O.FEAT_NAMES[j] for j in range(N_CMP_FEAT) if feat[i, j] != tfeat[a, j]]
                        raise AssertionError((q, int(docs[i]), bad, feat[i, :N_CMP_FEAT].tolist(), tfeat[a, :N_CMP_FEAT].tolist()))
                    assert ties[i] == tties[a], (q, a)
                    matched, total = int(tfeat[a, 2]), int(tfeat[a, 1])
                    if bits(base[i]) == bits(tbase[a]) or not 0 < matched < total:        # the base enters only a partial-coverage row's score
                        assert bits(sc[i]) == bits(tsc[a]), (q, int(docs[i]), "base", float(base[i]), "score", float(sc[i]), float(tsc[a]))
                    if bits(base[i]) != bits(tbase[a]):
                        assert not s1_exact, (q, int(docs[i]), "base", float(base[i]), float(tbase[a]))     # bit-exact Stage-1 rows: the same score / maxT
                        stats["base_mismatch"] += 1
                        gap = np.float32(1) - np.float32(matched) / np.float32(total)
                        slack = blend_slack(tsc[a], float(gap) * abs(float(base[i]) - float(tbase[a])))
                        if not score_matches(sc[i], tsc[a], True, slack, (q, int(docs[i]), "base", float(base[i]), float(tbase[a]))):
                            stats["s2_inexact"] += 1
        else:
            assert not r["used_coverage"], q
        # ---- final records
        gids = [x.document_id for x in got.records]
        if set(gids) != set(r["keys"]):
            stats["set_mismatch"] += 1
        else:
            os_ = dict(zip(r["keys"], [float(v) for v in r["scores"]]))
            for x in got.records:
                stats["max_final_abs"] = max(stats["max_final_abs"], abs(x.score - os_[x.document_id]))
            bad, swaps = assert_final_rows(gids, [x.score for x in got.records], r["keys"], r["scores"], stage2_scored(o, r), q)
            stats["final_inexact"] += bad
            if gids != r["keys"]:
                stats["order_mismatch"] += 1
    return stats


def test_ten_docs_full_parity(ten):
    e, o = ten
    qs = ["batman", "qick fux", "battamam", "new york", "speeding", "quik fox", "the fox", "fox", "gotham city crime", "wonder", "flash runs", "xyzabc", "a journey", "spider man"]
    st = compare_batch(e, o, qs, 10)
    assert st["set_mismatch"] == 0 and st["order_mismatch"] == 0, st


@pytest.fixture(scope="module", params=[(2, 30000, 10), (3, 20000, 20)], ids=["cfg2-30k", "cfg3-20k"])
def synth_pair(request):
    cfg, n, k = request.param
    s = Synth(cfg, docs=n)
    arena, offs = s.docs()
    e = gpu_engine(); e.index_flat(None, arena, offs, s.field_weights)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    return s, e, o, k


def test_synthetic_parity(synth_pair):
    s, e, o, k = synth_pair
    qa, qo = s.queries(300, qseed=11)
    st = compare_batch(e, o, Synth.texts(qa, qo), k)
    print("parity stats", st)
    assert st["feat_mismatch"] == 0
    assert st["set_mismatch"] == 0, st      # identical top-k DocumentId sets
    assert st["s1_boundary"] == 0, st       # exact replay: the Stage-1 top-`depth` SET is the oracle's for every query, ties included
    # an order difference is a swap of two rows whose oracle scores are one ulp apart, one of them not bit-equal (compare_batch asserts it)


def test_batching_is_transparent(synth_pair):
    s, e, o, k = synth_pair
    qa, qo = s.queries(64, qseed=5)
    qs = Synth.texts(qa, qo)
    a = e.search_batch(qs, k)
    b = [e.search_batch([q], k)[0] for q in qs[:16]]
    for x, y in zip(a[:16], b):
        assert [r.document_id for r in x.records] == [r.document_id for r in y.records]
        assert [r.score for r in x.records] == [r.score for r in y.records]   # deterministic, batch-independent


def test_sharded_equals_the_oracle():
    """Three doc-range shards (whole 65 536-id containers each; simulated on one GPU, numpy / torch ops in place of RCCL) against the ORACLE:
    global statistics + count all-reduce + first-pass lists + the exact Stage-1 replay across shards + owner-scored Stage 2.
    Host exchange buffers and device tensors (the RCCL code path) must agree bit for bit."""
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards, simulate_shards_dev
    from infidex_amd.engine import pack_texts
    from tests.parity_classify import assert_final_rows_match_oracle
    s = Synth(2, docs=180000)
    arena, offs = s.docs()
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    W = 3
    engs = [create_sharded_engine(r, W, 0) for r in range(W)]
    for e in engs:
        e.index_flat(None, arena, offs, s.field_weights)
    bases = [e.shard_info() for e in engs]
    assert [b for b, _ in bases] == [0, 65536, 131072] and sum(n for _, n in bases) == 180000      # container-aligned shards
    sess = [ShardSession(e) for e in engs]
    qa, qo = s.queries(200, qseed=21, fuzz=0.3)
    qs = Synth.texts(qa, qo) + ["qu", "zzzzqq", "the"]
    qs.append(" ".join(dict.fromkeys(w for t in qs[:40] for w in t.split())))      # > 32 distinct words: the long-query table travels through infx_shard_stage2 too
    assert len(qs[-1].split()) > 32
    a2, o2 = pack_texts(qs)
    host = simulate_shards(sess, a2, o2, 10)
    dev = simulate_shards_dev(sess, a2, o2, 10)
    for r in host[1:] + dev:                             # every rank ends with the same rows, whatever memory the exchange buffers live in
        for x, y in zip(r, host[0]):
            assert np.array_equal(x, y)
    k, sc, t, c, f = host[0]
    same, flips, inexact = assert_final_rows_match_oracle(k, sc, c, o, qs, 10, what="3 shards")
    replays = sum(x.s.last_timings()["exact_replays"] for x in sess)
    print("sharded vs oracle:", same, "identical order,", flips, "near-tie flips,", inexact, "rows not bit-equal; replayed on their owners:", replays)
    assert replays > 0                                   # the corpus has ambiguous cuts: the cross-shard replay really ran
    # the single index gives the same rows (both are the oracle's)
    ref = SearchEngine.create_default(device=0); ref.index_flat(None, arena, offs, s.field_weights)
    rk, rs, rt, rc, rf = ref.search_packed(a2, o2, 10)
    assert np.array_equal(rc, c)
    for i in range(len(qs)):
        assert set(rk[i, :int(rc[i])].tolist()) == set(k[i, :int(c[i])].tolist())


def test_sharded_sequential_chain_equals_the_parallel_replay(tmp_path):
    """INFX_EXACT_SLOW=1 sends every flagged query through the chained k_exact1 (one heap continued from shard to shard) instead of the parallel
    replay: the rows must be the same, and the oracle's."""
    import subprocess
    import sys
    script = r'''
import sys, numpy as np
from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards
from infidex_amd.engine import pack_texts
from tools.synth import Synth
s = Synth(2, docs=180000); arena, offs = s.docs()
engs = [create_sharded_engine(r, 2, 0) for r in range(2)]
for e in engs: e.index_flat(None, arena, offs, s.field_weights)
qa, qo = s.queries(120, qseed=21, fuzz=0.3)
a, o = pack_texts(Synth.texts(qa, qo))
k, sc, t, c, f = simulate_shards([ShardSession(e) for e in engs], a, o, 10)[0]
np.savez(sys.argv[1], k=k, sc=sc, t=t, c=c)
'''
    import os
    outs = []
    for slow in ("0", "1"):
        env = dict(os.environ); env["INFX_EXACT_SLOW"] = slow
        env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = str(tmp_path / f"r{slow}.npz")
        subprocess.run([sys.executable, "-c", script, out], check=True, env=env, timeout=900)
        outs.append(np.load(out))
    for key in ("k", "sc", "t", "c"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    from tests.parity_classify import assert_final_rows_match_oracle
    s = Synth(2, docs=180000); arena, offs = s.docs()
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    qa, qo = s.queries(120, qseed=21, fuzz=0.3)
    assert_final_rows_match_oracle(outs[1]["k"], outs[1]["sc"], outs[1]["c"], o, Synth.texts(qa, qo), 10, what="chained replay")


def test_long_documents_take_the_retry_launches():
    """Documents with more than 32 words are re-scored by the second k_stage2 launch (192-word tables in scratch), documents beyond 192 words by the third
    (tables in a global workspace: any text the reference accepts, Api/DocumentFields.cs:140): rows, features and scores must match the oracle whatever
    launch scored them.  A query beyond INFX_LONGQ_CHARS is answered as unsupported without failing its batch."""
    import random
    rng = random.Random(3)
    vocab = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel", "india", "juliet", "kilo", "lima", "mike",
             "november", "oscar", "papa", "quebec", "romeo", "sierra", "tango", "uniform", "victor", "whiskey", "xray", "yankee", "zulu"]
    docs = []
    for i in range(300):
        n = rng.choice([5, 12, 31, 32, 33, 40, 64, 100, 150, 190, 193, 260, 700])
        docs.append((i, " ".join(rng.choice(vocab) + (str(rng.randrange(30)) if rng.random() < 0.3 else "") for _ in range(n))))
    docs.append((300, " ".join(vocab[i % 26] + str(i) for i in range(2500))))                    # 2 500 distinct words
    docs.append((301, " ".join(rng.choice(vocab) + str(rng.randrange(400)) for _ in range(4000))))  # 4 000 words, many repeats
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    qs = ["alpha bravo", "charlie delta echo", "foxtrt golf", "hotel india12", "zulu", "november oscar papa quebec", "xray yankee", "kilo lima mik",
          "alpha0 bravo1", "zulu2495 alpha2496", "yankee2", "golf1410 hotel1411 india", "mike38 kilo", "whiskey399 tango"]
    res = e.search_batch(qs, 10)
    assert not any(r.unsupported or r.skipped_candidates for r in res)
    assert 300 in [x.document_id for x in res[9].records]                                           # the 2 500-word document is ranked for its own words
    st = compare_batch(e, o, qs, 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, st
    long_q = "alpha bravo " + " ".join("longishword%02d" % i for i in range(28))                     # 403 characters, 30 distinct words: inside the query envelope
    assert 400 < len(long_q) <= 512
    st = compare_batch(e, o, [long_q, "alpha bravo"], 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, st
    r = e.search_batch(["alpha bravo", "x" * 2100], 5)
    assert r[1].unsupported and not r[1].records and not r[0].unsupported and r[0].records       # beyond INFX_LONGQ_CHARS: unsupported, the batch goes on


def test_long_queries_take_the_long_query_launches():
    """The reference puts no limit on the query (CoverageEngine.cs:68).  Queries beyond 32 distinct words / 512 characters are scored by k_stage2's long-query
    launches (128-word tables, four mask words; documents beyond 192 words through the global-workspace pass): rows, features and scores must match the
    oracle for 40-, 100- and 128-word queries and a 600-character one, mixed with ordinary queries in one batch; only a query beyond 128 distinct words or
    2048 characters is answered as unsupported."""
    import random
    rng = random.Random(17)
    vocab = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel", "india", "juliet", "kilo", "lima", "mike",
             "november", "oscar", "papa", "quebec", "romeo", "sierra", "tango", "uniform", "victor", "whiskey", "xray", "yankee", "zulu"]
    word = lambda: rng.choice(vocab) + (str(rng.randrange(40)) if rng.random() < 0.5 else "")
    docs = []
    for i in range(400):
        n = rng.choice([5, 12, 31, 33, 40, 64, 100, 150, 190, 193, 260, 700])
        docs.append((i, " ".join(word() for _ in range(n))))
    docs.append((400, " ".join(vocab[i % 26] + str(i) for i in range(2500))))                       # 2 500 distinct words: the global-workspace pass
    long1 = " ".join(vocab[i % 26] + str(i) for i in range(100))                                       # 100 distinct words, all of document 400
    docs.append((401, long1))                                                                          # ... and a document that IS the query
    docs.append((402, " ".join(vocab[i % 26] + str(i) for i in range(0, 200, 2))))
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    q40 = " ".join(vocab[i % 26] + str(i % 40) for i in range(40))
    q40typo = " ".join((vocab[i % 26][:-1] + "x" if i % 7 == 3 else vocab[i % 26]) + str(i % 40) for i in range(40))      # some words one edit away
    q128 = " ".join(vocab[i % 26] + str(i) for i in range(128))
    q600 = " ".join(["alphabravocharliedeltaechofoxtrotgolfhotelindiajulietkilolimamike" + str(i) for i in range(9)]) + " alpha bravo"
    q33 = " ".join(vocab[i % 26] + str(i) for i in range(33))                                          # one word beyond the fast envelope
    assert len(q600) > 512 and len(set(q128.split())) == 128 and len(q128) <= 2048
    qs = ["alpha bravo", q40, "charlie delta echo", long1, q40typo, q128, q600, "zulu2495 alpha2496", q33, long1 + " " + long1.split()[0]]
    res = e.search_batch(qs, 10)
    assert not any(r.unsupported or r.skipped_candidates for r in res), [(r.unsupported, r.skipped_candidates) for r in res]
    assert res[3].records[0].document_id == 401                                                        # the document that is the 100-word query comes first
    st = compare_batch(e, o, qs, 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, st
    # the same long queries alone and in another order: batching is transparent for them too
    st = compare_batch(e, o, [q128, q40], 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, st
    # beyond the long envelope: unsupported, the rest of the batch is answered
    q129 = q128 + " zulu9999"
    r = e.search_batch([q129, "alpha bravo", "x" * 2049, q40], 5)
    assert r[0].unsupported and not r[0].records and r[2].unsupported and not r[2].records
    assert not r[1].unsupported and r[1].records and not r[3].unsupported and r[3].records
    assert [x.document_id for x in r[3].records] == o.search(q40, 5)["keys"]


def test_queries_beyond_64_reference_terms_take_the_exact_cut():
    """A query of 40 words carries more than 64 reference terms (words + n-grams, up to 128: VectorModel.cs:381): its rows take four mask words and the sequential
    replay (k_mark_wide, k_exact1 reading the masks from the arena).  The corpus repeats every text 2 .. 30 times, so the Stage-1 scores form plateaus across
    the cuts at depths 40, 7 and 3: with the first-pass cut (k_select by document id, rounds 2-5) the SET differs from the oracle's heap at some of them; with the replay
    it is the oracle's for every query — narrow queries of the same batch (parallel replay over the first two words of four) included."""
    import random
    rng = random.Random(23)
    vocab = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel", "india", "juliet", "kilo", "lima", "mike",
             "november", "oscar", "papa", "quebec", "romeo", "sierra", "tango", "uniform", "victor", "whiskey", "xray", "yankee", "zulu"]
    texts = []
    for i in range(160):
        n = rng.choice([3, 5, 8, 12, 20, 40])
        texts.append(" ".join(rng.choice(vocab) + (str(rng.randrange(12)) if rng.random() < 0.4 else "") for _ in range(n)))
    docs = []
    for t in texts:
        for _ in range(rng.choice([2, 3, 5, 11, 30])): docs.append((len(docs), t))
    rng.shuffle(docs); docs = [(i, t) for i, (_, t) in enumerate(docs)]
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    q40 = " ".join(vocab[i % 26] + (str(i % 12) if i % 3 == 0 else "") for i in range(40))
    q60 = " ".join(vocab[(7 * i) % 26] + (str(i % 12) if i % 2 else "") for i in range(60))
    wide = [q40, q60, q40 + " zulu7", " ".join(texts[i] for i in (3, 9, 27))]
    qs = ["alpha bravo", wide[0], "charlie delta echo", wide[1], "golf hotel india juliet kilo lima mike november", texts[5], wide[2], wide[3]]
    for depth in (40, 7, 3):
        st = compare_batch(e, o, qs, 10, depth=depth)
        assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0 and st["s1_boundary"] == 0, (depth, st)
        assert st["s1_bitexact"] == len(qs), (depth, st)
    # the test bites: without the replay (the first-pass cut by document id, what such queries got before) some of these cuts are not the oracle's ...
    u = gpu_engine(exact_replay=False); u.index_documents([Document(k, t) for k, t in docs])
    bites = sum(compare_batch(u, o, wide, 10, depth=d, check_features=False)["s1_boundary"] for d in (40, 7, 3))
    assert bites > 0
    # ... and every wide query alone in its batch (no narrow query: four mask words for nobody else) is replayed and right
    replays = 0
    for q in wide:
        st = compare_batch(e, o, [q], 10, depth=7)
        assert st["s1_boundary"] == 0 and st["s1_bitexact"] == 1 and st["set_mismatch"] == 0, st
        replays += e.last_timings()["exact_replays"]
    assert replays >= 2, replays


def test_long_tokens_have_no_length_limit():
    """Tokens far longer than any fixed cost row: the Levenshtein band (k_stage2) lives in registers, so 70-150 character words in documents
    and queries (exact, one typo, prefix, joined) are scored like the reference does — no envelope on the token length any more."""
    import random
    rng = random.Random(5)
    alpha = "abcdefghijklmnopqrstuvwxyz"
    longw = ["".join(rng.choice(alpha) for _ in range(n)) for n in (70, 85, 100, 120, 150, 64, 63, 65)]
    docs = []
    for i in range(120):
        ws = [rng.choice(longw) for _ in range(rng.choice([1, 2, 3]))] + [rng.choice(["alpha", "bravo", "charlie", "delta"]) for _ in range(rng.choice([0, 1, 2]))]
        rng.shuffle(ws)
        docs.append((i, " ".join(ws)))
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)

    def typo(w):
        p = rng.randrange(5, len(w) - 5); return w[:p] + ("x" if w[p] != "x" else "y") + w[p + 1:]
    qs = [longw[0], longw[1] + " alpha", typo(longw[2]), typo(longw[3]) + " bravo", longw[4][:90], longw[0] + longw[1], typo(longw[5]), longw[6] + " " + typo(longw[7]),
          longw[2][:60] + " " + longw[3][:40]]
    qs = [q for q in qs if len(q) <= 250]
    st = compare_batch(e, o, qs, 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0 and st["s1_boundary"] == 0, st
    assert not any(r.unsupported or r.skipped_candidates for r in e.search_batch(qs, 10))


def test_deleted_documents_are_skipped_like_the_reference():
    """Document.Deleted after indexing (DocumentCollection.DeleteDocumentsByKey): postings / df / avgdl keep the document, the query path skips
    it — never in the Stage-1 heap (Bm25Scorer.cs:322-323), never scored by Stage 2 (SearchPipeline.cs:463-465), no docIndex for a deleted
    WordMatcher id (:532-537) which still uses up a WordMatcher-only slot (:387-397).  Engine vs oracle with the same deletions: identical
    Stage-1 sets, the same Stage-2 evaluations (features bit-exact) and the same final lists."""
    import random
    rng = random.Random(11)
    vocab = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel", "india", "juliet", "kilo", "lima", "mike",
             "november", "oscar", "papa", "quebec", "romeo", "sierra", "tango", "uniform", "victor", "whiskey", "xray", "yankee", "zulu"]
    docs = [(i, " ".join(rng.choice(vocab) + (str(rng.randrange(6)) if rng.random() < 0.3 else "") for _ in range(rng.choice([2, 3, 5, 8, 13])))) for i in range(600)]
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    qs = ["alpha bravo", "charlie delta echo", "foxtrt golf", "hotel india1", "zulu", "november oscar papa quebec", "xray yankee", "kilo lima mik",
          "zul", "whiskei", "tango3 uniform", "victor victor", "romeo sierra tango uniform victor", "mike2", "juliet0 kilo", "alpa brvo", "echo5"]
    before = [[x.document_id for x in r.records] for r in e.search_batch(qs, 10)]
    # delete a third of the corpus, and on top of it the current best two rows of every query (so the deletions certainly matter)
    gone = set(rng.sample(range(600), 200))
    for ids in before:
        gone.update(ids[:2])
    assert e.delete_documents(sorted(gone)) == len(gone) and o.delete_keys(sorted(gone)) == len(gone)
    assert e.delete_documents(sorted(gone)) == 0                                     # already marked
    st = compare_batch(e, o, qs, 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0 and st["s1_boundary"] == 0, st
    after = [[x.document_id for x in r.records] for r in e.search_batch(qs, 10)]
    assert not any(set(ids) & gone for ids in after) and any(after)
    # small depths: the WordMatcher-only limit counts deleted ids (wmLimit), docIndex 0/1 skip them
    for depth in (1, 2, 3, 7):
        res = e.search_batch(qs, 5, depth)
        for q, r in zip(qs, res):
            assert sorted(x.document_id for x in r.records) == sorted(o.search(q, 5, depth)["keys"]), (q, depth)
    # deleting everything that matches leaves nothing; restoring brings the first answer back
    e.restore_documents()
    assert [[x.document_id for x in r.records] for r in e.search_batch(qs, 10)] == before
    e.delete_documents(range(600))
    assert all(not r.records for r in e.search_batch(qs, 10))


def test_depth_and_result_count_variants(ten):
    e, o = ten
    qs = ["the fox", "batman", "quick", "city", "new york city"]
    for k, depth in ((1, 500), (3, 500), (10, 4), (2, 2), (10, 1)):
        res = e.search_batch(qs, k, depth)
        for q, r in zip(qs, res):
            ro = o.search(q, k, depth)
            assert [x.document_id for x in r.records] == ro["keys"], (q, k, depth)
    # blank / whitespace / too-short queries inside a batch do not disturb their neighbours
    res = e.search_batch(["", "   ", "a", "batman", "qick fux"], 10)
    assert [len(r.records) for r in res[:3]] == [0, 0, 0]
    assert [x.document_id for x in res[3].records][0] == 6 and [x.document_id for x in res[4].records] == [5, 1]


def test_batches_without_any_index_term():
    """A batch whose queries hit no index term at all (nd == 0): no Stage-1 launch, coverage still runs on WordMatcher candidates."""
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in TEN_DOCS])
    o = O.OracleEngine.create_default(); o.index(TEN_DOCS)
    qs = ["zzzzqqq", "xq", "", "wwwwvvvv kkkkjjjj"]
    res = e.search_batch(qs, 10)
    for q, r in zip(qs, res):
        assert [x.document_id for x in r.records] == o.search(q, 10)["keys"], q


def test_query_with_more_wordmatcher_lists_than_the_device_limit():
    """A 30-word query produces more WordMatcher lists than INFX_MAX_WM_LISTS (256): the host merges them into one list; results match the oracle."""
    import random
    rng = random.Random(11)
    words = ["".join(rng.choice("abcdefghij") for _ in range(rng.choice([4, 5, 6, 7]))) for _ in range(400)]
    docs = [(i, " ".join(rng.choice(words) for _ in range(rng.choice([6, 10, 14])))) for i in range(3000)]
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    q = " ".join(words[i] for i in range(0, 300, 10))          # 30 distinct index words
    st = compare_batch(e, o, [q, "abcd efgh", q[: len(q) // 2]], 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, st


def test_random_unicode_corpora_full_parity():
    """End to end on random text with diacritics, mixed case, all delimiters, odd whitespace, empty / one-character / duplicate documents."""
    from tests import unicode_corpus
    for seed in range(3):
        docs, queries = unicode_corpus.make(seed, ndocs=600, nqueries=80)
        e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
        o = O.OracleEngine.create_default(); o.index(docs)
        st = compare_batch(e, o, queries, 10)
        assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, (seed, st)


def test_scripts_beyond_latin1_full_parity():
    """Vietnamese, Latin Extended-B, accented / final-sigma Greek, Cyrillic beyond U+045F, Armenian, Georgian, full-width Latin, Cherokee, and the
    characters OrdinalIgnoreCase equates with another lower-case letter: rows, scores and every Stage-2 feature equal the oracle's, whose case mappings
    and letter set come from the same Unicode data as the product's (tools/gen_unicode_tables.py) and which compares per site as the reference does
    (ToUpperInvariant images for OrdinalIgnoreCase, ToLowerInvariant where the reference lower-cases)."""
    from tests import unicode_corpus
    for si, script in enumerate(sorted(unicode_corpus.SCRIPTS)):
        docs, queries = unicode_corpus.make_script(si, script, ndocs=300, nqueries=50)
        e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
        o = O.OracleEngine.create_default(); o.index(docs)
        st = compare_batch(e, o, queries, 10)
        assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, (script, st)


def test_ordinal_ignore_case_aliases():
    """Where an alias character meets its base letter.  OrdinalIgnoreCase compares ToUpperInvariant images, so a document word 'λογοσκοπος' starts with the query word
    'λογος' (final sigma and sigma share the capital), 'ſtraße' equals 'straße', 'µm' equals 'μm' — while the reference's ToLowerInvariant / ordinal sites (the LCS,
    the transposition scan of CalculateDamerau, FusionSignalComputer.cs:191-228, 427, 457-550, FuzzyWordMatcher.cs:110) see alias and base as DIFFERENT characters.
    Round 6: Stage 2 runs its ALIAS instantiation for such corpora / queries and compares per site as the reference does: returned documents, final scores and every
    integer feature equal the oracle's (rounds 4-5 folded the texts and only the documents were compared)."""
    docs = [(1, "λογοσκοπος αλφα"), (2, "λογος βητα"), (3, "ſtraße lang"), (4, "straße kurz"), (5, "10 µm filter"), (6, "10 μm sieve"), (7, "unrelated text here"),
            (8, "ΛΟΓΟΣ ΚΕΦΑΛΑΙΑ"), (9, "ϑερμος ϕως"), (10, "θερμος φως"), (11, "λογοσ λογος λογοι"), (12, "κοσμος κοσμοσ κοςμος"), (13, "οδυσσευς οδυσσευσ ταξιδι")]
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    queries = ["λογος", "λογοσ", "straße", "ſtraße", "µm filter", "μm sieve", "θερμος", "ϑερμος φως", "ΛΟΓΟΣ", "κοσμος", "κοσμοσ", "οδυσσευς ταξιδι", "λογοσ λογοι", "κοςμος κοσμος"]
    for q in queries:
        got = [x.document_id for x in e.search(q, 10).records]
        want = o.search(q, 10)["keys"]
        assert sorted(got) == sorted(want), (q, got, want)
    st = compare_batch(e, o, queries, 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, st


def test_alias_characters_in_the_queries_only():
    """The corpus holds no alias character (the plain Stage-2 instantiation would do) but a query does: the batch runs the ALIAS instantiation — 'λογος' against a
    document 'λογοσ' differs at the lower-case sites.  Rows, scores, features equal the oracle's; a batch without such a query runs the plain instantiation again."""
    docs = [(1, "λογοσ βητα"), (2, "κοσμοσ αλφα"), (3, "λογοσκοποσ γαμμα"), (4, "plain latin text"), (5, "ταξιδι κοσμοσ λογοσ")]
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    for queries in (["λογος", "κοσμος λογος", "plain text", "λογοσκοπος"], ["λογοσ", "plain latin", "κοσμοσ ταξιδι"]):
        st = compare_batch(e, o, queries, 10)
        assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0, (queries, st)


ASTRAL_DOCS = [(1, "\U0001F50Dab zeta"), (2, "\U0001F50Eab yotta"), (3, "plain \U0001F50Dab"), (4, "x\U0001F50D \U0001F50Ex \U0001F50Dab"), (5, "\U0001F50D"),
               (6, "\U00020000\U00020001 cjk\U00020001"), (7, "�ab already replaced"), (8, "x\U00020000 end"), (20, "emoji \U0001F600\U0001F601 party \U0001F600"),
               (21, "\U0001D49C\U0001D4B7\U0001D4B8 math script"), (22, "mixed a\U0001F50Db c\U0001F50Ed"), (23, "\ud83d lone high"), (24, "lone low \udd0d tail")]
ASTRAL_QUERIES = ["\U0001F50Dab", "\U0001F50Eab zeta", "a\U0001F50Db", "emoji \U0001F600", "\U0001D49C\U0001D4B7\U0001D4B8", "x\U0001F50D", "\U0001F50Dxb", "cjk\U00020001",
                  "party \U0001F601\U0001F600", "\U0001F50Dab\U0001F50E", "\ud83d lone", "low \udd0d", "math script", "mixed"]


def test_characters_outside_the_bmp_on_gpu():
    """Surrogate pairs and lone surrogates through the whole device pipeline (k_wm, k_ld1, k_stage2 work on UTF-16 code units like the reference): rows and
    scores equal the oracle's.  Staged in round 4 without GPU time; first run on an MI355X in round 5 (green).  The host side is covered on CPU by
    test_host_parity.py::test_characters_outside_the_bmp_index_and_plan_like_the_oracle; the reference's PersistenceTests index U+1F50D."""
    o = O.OracleEngine.create_default(); o.index(ASTRAL_DOCS)
    e = SearchEngine.create_default(device=0); e.index_documents([Document(k, t) for k, t in ASTRAL_DOCS])
    for q, r in zip(ASTRAL_QUERIES, e.search_batch(ASTRAL_QUERIES, 10)):
        w = o.search(q, 10)
        if w["unsupported"]:
            assert r.records == [] or len(r.records) == 0, q
            continue
        assert [x.document_id for x in r.records] == w["keys"], (q, r.records, w)
        assert_final_rows(w["keys"], [x.score for x in r.records], w["keys"], w["scores"], stage2_scored(o, w), q)


def test_high_term_frequencies():
    """Documents that repeat a word up to 150 times: byte tf values from 2 to ~190 (Term.cs:87-109).  The replay kernels get tf >= 3 through the
    per-row exception records (k_accumulate) or the posting-list lookup."""
    import random
    rng = random.Random(9)
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    docs = []
    for i in range(400):
        w = rng.choice(words); reps = rng.choice([1, 2, 3, 5, 14, 15, 16, 40, 90, 150])
        docs.append((i, " ".join([w] * reps + [rng.choice(words) for _ in range(rng.randrange(0, 4))])))
    e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    st = compare_batch(e, o, ["alpha", "bravo charlie", "delta echo foxtrot", "golf hotel", "alpha alpha", "hotl", "charlie delta"], 10)
    assert st["set_mismatch"] == 0 and st["feat_mismatch"] == 0 and st["s1_boundary"] == 0, st


def test_accumulate_schedules_agree_bit_for_bit(tmp_path):
    """Stage-1 accumulation is the same arithmetic in the same order whichever kernel takes a (query, stripe) pair and however the blocks are scheduled: the sparse
    kernel (k_accumulate_sparse: candidates look their postings up) for stripes of <= INFX_ACC_SPARSE_T candidates and the streaming kernel (k_accumulate: byte scatter
    + probe per (list, range)) for the rest, or the streaming kernel alone with the XCD-aware block map or the query-fastest one (INFX_ACC_SKIP=32) and stripes of
    1 / 2 / 8 doc ranges per wave.  Likewise k_select's cut, whether a query's rows are swept by its own workgroup or by several in front of it (k_selg_*).
    Final rows, fp32 scores and the Stage-1 rows (ids and score bits) of a fuzzy batch must be identical, with deletions too.  (Until round 6 this test also held the alternative accumulation designs — mask scatter, probe-pool-score, 4-bit cells,
    container mailbox, and round 6's search kernel; all bit-identical, none faster, all deleted: HISTORY.md.)"""
    import os
    import subprocess
    import sys
    script = r'''
import sys, numpy as np
from infidex_amd import SearchEngine
from infidex_amd.engine import pack_texts
from tools.synth import Synth
s = Synth(3, docs=60000); arena, offs = s.docs()
e = SearchEngine.create_default(device=0, want_features=True); e.index_flat(None, arena, offs, s.field_weights)
qa, qo = s.queries(400, qseed=33, fuzz=0.5)
texts = Synth.texts(qa, qo) + ["qu", "", "zzzzqq", "the of and"]
a, o = pack_texts(texts)
out = {}
for tag in ("plain", "deleted"):
    if tag == "deleted": e.delete_documents(np.arange(0, 60000, 7))
    k, sc, t, c, f = e.search_packed(a, o, 20)
    s1 = [e.last_stage1(i) for i in range(0, len(texts), 5)]
    out[tag + "_k"] = k; out[tag + "_sc"] = sc; out[tag + "_t"] = t; out[tag + "_c"] = c; out[tag + "_f"] = f
    out[tag + "_s1k"] = np.concatenate([x[0] for x in s1]); out[tag + "_s1s"] = np.concatenate([x[1] for x in s1]).view(np.uint32)
np.savez(sys.argv[1], **out)
'''
    res = []
    variants = [dict(),                                                        # shipping split: stripes of <= 64 candidates search, the rest stream
                dict(INFX_ACC_SPARSE_T="0"), dict(INFX_ACC_SPARSE_T="8"), dict(INFX_ACC_SPARSE_T="33"), dict(INFX_ACC_SPARSE_T="150"), dict(INFX_ACC_SPARSE_T="4096"),      # one kernel (streaming) / other split points (beyond 64: several rounds per stripe)
                dict(INFX_ACC_SPARSE_T="0", INFX_ACC_SKIP="32"), dict(INFX_ACC_SPARSE_T="0", INFX_ACC_STRIPE="1"), dict(INFX_ACC_SPARSE_T="0", INFX_ACC_STRIPE="2"), dict(INFX_ACC_SPARSE_T="0", INFX_ACC_STRIPE="8"),
                # k_select: the largest queries swept by several workgroups (k_selg_hist / k_selg_gather) from 64 / 3000 rows on (default 65536: none at this size), or never
                dict(INFX_SEL_GIANT_MIN="64"), dict(INFX_SEL_GIANT_MIN="3000"), dict(INFX_SEL_GIANT_MIN="0"),
                # k_accumulate's block order: the (up to 64) queries of >= 2000 / 20000 possible rows take all their stripes first, or plain query order (default 393216 rows: none at this size, queries by row bound)
                dict(INFX_ACC_HEAVY_ROWS="2000"), dict(INFX_ACC_HEAVY_ROWS="20000", INFX_ACC_SPARSE_T="0"), dict(INFX_ACC_HEAVY_ROWS="0")]
    for vi, var in enumerate(variants):
        env = dict(os.environ); env.update(var)
        env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = str(tmp_path / f"acc{vi}.npz")
        subprocess.run([sys.executable, "-c", script, out], check=True, env=env, timeout=900)
        res.append(np.load(out))
    assert len(res[0].files) == 14
    for other in res[1:]:
        for key in res[0].files:
            assert np.array_equal(res[0][key], other[key]), key
    assert res[0]["plain_s1k"].size > 1000


def test_expansion_cache_eviction_inside_a_batch():
    """More than 1000 distinct misspelt words in ONE batch, the first queries repeated at its end: by then the LRU expansion cache (1000 entries, as the
    reference's) has evicted their words, so two queries of the batch hold different union objects for one word.  The batch still builds ONE device
    union per word, in the same order on every shard (its cardinality is all-reduced position by position), and the rows are the oracle's — on one GPU
    and on two document shards."""
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards
    from infidex_amd.engine import pack_texts
    from tests.parity_classify import assert_final_rows_match_oracle
    s = Synth(2, docs=70000)
    arena, offs = s.docs()
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    qa, qo = s.queries(1500, qseed=61, fuzz=1.0)           # ~1 230 distinct misspelt words
    qs = Synth.texts(qa, qo)
    qs = qs + qs[:60]
    a2, o2 = pack_texts(qs)
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    k, sc, t, c, f = e.search_packed(a2, o2, 10)
    assert e.fuzzy_cache_size() == 1000                       # the batch overflowed the cache
    same, flips, inexact = assert_final_rows_match_oracle(k, sc, c, o, qs, 10, what="one GPU")
    print("one GPU vs oracle:", same, "identical order,", flips, "near-tie flips,", inexact, "rows not bit-equal")
    assert np.array_equal(k[:60], k[-60:]) and np.array_equal(c[:60], c[-60:])      # a repeated query gets the rows of its first occurrence
    W = 2
    engs = [create_sharded_engine(r, W, 0) for r in range(W)]
    for g in engs:
        g.index_flat(None, arena, offs, s.field_weights)
    sess = [ShardSession(g) for g in engs]
    host = simulate_shards(sess, a2, o2, 10)
    for r in host[1:]:
        for x, y in zip(r, host[0]):
            assert np.array_equal(x, y)
    assert np.array_equal(host[0][0], k) and np.array_equal(host[0][3], c)


def test_segmented_documents_on_gpu():
    """SegmentTrackingTests.cs:92-210, 324-345: several documents under one DocumentKey.  One row per key (ConsolidateSegments), and — the part the reference's
    assertions do not see but its code does — Stage 2 scores a key through GetDocumentByPublicKey, i.e. with the text of the key's FIRST document and the best
    segment's BM25 share: keys AND scores equal the oracle's, for the reference's queries and for queries that hit several segments of one key."""
    from tests.test_oracle_kats import SEGMENT_CASES
    extra = {0: ["summary animals"], 1: ["chapter one", "batman robin"], 2: ["the dog"], 4: ["hero journey"], 5: ["segment text"]}
    for i, (docs, q, want) in enumerate(SEGMENT_CASES):
        o = O.OracleEngine.create_default(); o.index(docs)
        e = gpu_engine(); e.index_documents([Document(k, t) for k, t in docs])
        queries = [q] + extra.get(i, [])
        for text, r in zip(queries, e.search_batch(queries, 10)):
            w = o.search(text, 10)
            assert [x.document_id for x in r.records] == w["keys"], (text, r.records, w)
            assert_final_rows(w["keys"], [x.score for x in r.records], w["keys"], w["scores"], stage2_scored(o, w), text)
        assert sorted(x.document_id for x in e.search_batch([q], 10)[0].records) == want
