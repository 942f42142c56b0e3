"""tests/replay_model.py pinned on the CPU.  (1) The model IS the reference's reading: on two corpora its heap content equals the oracle's Stage-1 rows, document for
document and score bit for score bit, so that what tests/test_gpu_replay_plateaus.py holds the replay kernels to is Bm25Scorer.Search and not the model's own idea
of it.  (2) The constructed index bites: every query of replay_model.plateau_batch is a structural plateau across the cut at every depth, with and without the
deletions, and each of the model's five deliberate misreadings changes the result of at least one of them."""
import numpy as np
import pytest

from tests import oracle_lib as O
from tests import replay_model as RM
from tests import stage1_model as M
from tools.synth import Synth

SKIP_CAP = 0.10                                            # tests/test_stage1_model.py's
NQ, QSEED = 150, 17


def _bits(keys, scores):
    return {int(k): int(v) for k, v in zip(keys.tolist(), np.asarray(scores, np.float32).view(np.uint32).tolist())}


def _against_the_oracle(o, queries, what):
    """queries: (text, depth).  Returns the totals of what the model reported over the checked queries."""
    ex = o.export_index()
    po, pd, pw = ex["post_off"], ex["post_doc"], ex["post_w"]
    ix = M.Index(ex["doc_len"], np.float32(o.avgdl))
    assert ix.N == o.num_docs
    skipped = checked = 0
    tot = dict(chunks=0, skipped=0, tail_postings=0, tied_evictions=0, equal_arrivals=0)
    for q, depth in queries:
        o.search(q, 10, depth)
        tid, df, idf, mx = o.last_terms()
        st = o.last_stats()
        ok, osc = o.last_stage1()
        if len(tid) == 0:
            assert len(ok) == 0
            continue
        if (tid < 0).any():                                 # a fuzzy virtual term: its doc set is not in the exported arrays
            skipped += 1
            continue
        terms = [M.Term(pd[int(po[t]):int(po[t + 1])], pw[int(po[t]):int(po[t + 1])], i, d) for t, d, i in zip(tid.tolist(), df.tolist(), idf.tolist())]
        ql = q.lower()
        P = M.plan(ix, terms, depth, [o.prefix_docset(ql[:n]) for n in range(min(len(ql), 3), 0, -1)])
        if P.ambiguous:
            skipped += 1
            continue
        checked += 1
        assert P.mode == st["mode"] and int(P.cand.sum()) == st["candidates"], (what, q, P.mode, int(P.cand.sum()), st)
        assert [float(RM.max_score32(t.idf, ix.avgdl)) for t in terms] == [float(x) for x in mx], (what, q, "maxScore")
        R = RM.replay(ix, terms, P.cand, depth, max_scores=mx)
        want = _bits(ok, osc)                               # internal id == DocumentKey here
        assert set(R.result) == set(want), (what, q, depth, "documents", sorted(set(R.result) ^ set(want))[:10])
        wrong = {d: (hex(R.result[d]), hex(want[d])) for d in want if R.result[d] != want[d]}
        assert not wrong, (what, q, depth, "score bits", len(wrong), list(wrong.items())[:5])
        for k in tot:
            tot[k] += getattr(R, k)
    share = skipped / len(queries)
    print(f"replay model vs oracle, {what}: {checked} queries checked bit for bit, {skipped} skipped ({100 * share:.1f} %); over the batch {tot}")
    assert share <= SKIP_CAP, (what, skipped, len(queries))
    return tot


def test_model_equals_the_oracle_on_the_synthetic_corpus():
    s = Synth(2, docs=20000)
    arena, offs = s.docs()
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    qa, qo = s.queries(NQ, qseed=QSEED, fuzz=0.0)
    _against_the_oracle(o, [(q, 500) for q in Synth.texts(qa, qo)], "Synth(2, docs=20000)")


def test_model_equals_the_oracle_on_the_tie_corpus():
    """More than 131 072 short documents from a few dozen templates: thousands share length and matched terms.  The batch must have exercised the rules."""
    from infidex_amd.engine import pack_texts
    texts, queries = RM.tie_corpus()
    assert len(texts) > 131072 and {d for _, d in queries} == set(RM.TIE_DEPTHS)
    arena, offs = pack_texts(texts)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs); o.finalize()
    tot = _against_the_oracle(o, queries, "tie corpus")
    assert tot["tied_evictions"] > 0 and tot["skipped"] > 0 and tot["tail_postings"] > 0, tot


@pytest.fixture(scope="module")
def plateau():
    return RM.PlateauIndex()


def test_constructed_index_is_what_it_says(plateau):
    P = plateau
    assert P.N == 2 * 65536 + 9000 and len(np.unique(P.doc_len)) == 4 and set(np.unique(P.post_w).tolist()) == {1, 2, 3, 7, 255}
    assert len(set(P.df.tolist())) == P.T
    # the two formulas differ in the last bit for TAIL's (tf, length) and for PURE's tf 1 at another length: picked by the model
    tail = P.term("TAIL")
    pairs = RM.differing_pairs(tail.idf, RM.TFS, P.lengths, P.avgdl)
    assert (P.tail_tf, float(P.lengths[0])) in pairs and len(pairs) < 20, pairs
    print("lengths", P.lengths.tolist(), "avgdl", float(P.avgdl), "(tf, length) pairs the formulas round differently at TAIL's idf:", pairs)
    # container populations and chunk sizes of the single-list queries
    pop = lambda name: np.bincount(P.lists[P.id[name]] >> 16, minlength=3).tolist()
    assert [pop(n) for n in ("CA", "CB", "CC", "CD", "CE")] == [[1, 0, 4095], [1, 1, 4096], [4097, 1, 8193], [256, 257, 1024], [4096 + 256, 4096 + 257, 1025]]
    ids = set(np.concatenate([P.lists[P.id[n]] for n in ("CA", "CB", "CC")]).tolist())
    assert {65535, 65536, 131071, 131072} <= ids
    # TAIL's matches per chunk of "tails 0..7": every residue mod 8, one count below 8
    Q = next(q for q in RM.plateau_batch(P) if q["name"] == "tails 0..7")
    ix, terms, pl, ms = RM.plateau_model(P, Q, 500)
    docs = np.flatnonzero(pl.cand)
    per = np.bincount(np.searchsorted(docs, tail.docs) // RM.CHUNK + 100 * (tail.docs >> 16))
    per = per[per > 0]
    assert set((per % 8).tolist()) == set(range(8)) and per.min() < 8, per.tolist()
    # three tf >= 3 terms in one row; mask widths of one, two and four words
    assert [int(P.term("X%d" % j).tf[0]) for j in range(3)] == [3, 7, 255]
    assert sorted(len(q["terms"]) + q["virt"] for q in RM.plateau_batch(P))[-2:] == [40, 70] and any(len(q["terms"]) == 3 for q in RM.plateau_batch(P))


@pytest.mark.parametrize("deleted", (False, True), ids=["all documents", "after the deletions"])
def test_every_fixture_query_is_a_plateau_across_the_cut(plateau, deleted):
    """What makes k_select flag the query for an exact plateau: more rows than depth, rows of bit-equal first-pass score on both sides of the (score, doc) cut, and
    no dependence on the order of equal idfs — at every depth the GPU test runs."""
    P = plateau
    for depth in RM.DEPTHS:
        for Q in RM.plateau_batch(P):
            ix, terms, pl, ms = RM.plateau_model(P, Q, depth, deleted)
            assert not pl.ambiguous, (Q["name"], depth)
            rows, tied = RM.plateau_at_cut(ix, terms, pl.cand, depth)
            assert rows >= depth + 1 and tied, (Q["name"], depth, rows, tied)


def test_fixture_cases_bite(plateau):
    """The named cases do what their names say, by the model's own report."""
    P = plateau
    rep = {}
    for Q in RM.plateau_batch(P):
        ix, terms, pl, ms = RM.plateau_model(P, Q, 500, True)
        rep[Q["name"]] = RM.replay(ix, terms, pl.cand, 500, ms)
    assert rep["pure plateau"].tail_postings == 0 and rep["pure plateau"].equal_arrivals > 0 and rep["pure plateau"].tied_evictions == 0
    assert rep["rising plateau"].tied_evictions > 1000                                   # (nearly) every arrival evicts one of several tied minima
    assert rep["falling plateau"].tied_evictions == 0 and len(rep["falling plateau"].result) == 500      # fills once, then refuses
    assert rep["arrival equals threshold"].equal_arrivals > 0
    assert rep["tails 0..7"].tail_postings > 0
    ms = rep["maxscore skips"]
    th = [float(x) for x in ms.thresholds]
    assert ms.skipped > 0 and th == sorted(th) and len(set(th)) >= 4, (ms.skipped, sorted(set(th)))      # a threshold that rises from chunk to chunk
    assert rep["containers 4097/1/8193"].chunks == 6 and rep["chunks 256/257/1024"].chunks == 3
    # the 100 x depth stop of the disjunctive walk falls inside the term list at the small depths
    stop = next(q for q in RM.plateau_batch(P) if q["name"] == "100 x depth stop")
    cands = [int(RM.plateau_model(P, stop, d)[2].cand.sum()) for d in (1, 64, 500)]
    assert cands == [9000, 9000, 60000], cands
    # "refused interval" at depths 1 and 2: container 0 fills the heap with tail-formula rows, so the exact threshold at the next chunk lies one ulp above the
    # threshold predicted from first-pass scores, and REFB's turn (cur + a bound that adds nothing) has rows whose cur lies on either side
    ref = next(q for q in RM.plateau_batch(P) if q["name"] == "refused interval")
    for depth in (1, 2):
        ix, terms, pl, ms = RM.plateau_model(P, ref, depth)
        R = RM.replay(ix, terms, pl.cand, depth, ms)
        docs, fp = RM.first_pass(ix, terms[:1], pl.cand)
        lane = np.float32(fp[0])
        assert len(set(fp.tolist())) == 1 and float(ms[1]) == float(np.float32(RM.TINY_BOUND)) and np.float32(lane + ms[1]) == lane
        assert R.chunks == 2 and R.thresholds[1] == np.nextafter(lane, np.float32(np.inf)) and R.skipped == 50, (depth, R.thresholds, lane, R.skipped)
        assert all(d < RM.C1 for d in R.result) and len(R.result) == depth
    print({n: dict(chunks=r.chunks, skipped=r.skipped, tail=r.tail_postings, tied_evictions=r.tied_evictions, equal_arrivals=r.equal_arrivals) for n, r in rep.items()})


def test_every_misreading_changes_a_fixture_query(plateau):
    """Each of the five misreadings of replay_model.MISREADINGS changes the result (set or bits) of at least one query of the batch."""
    P = plateau
    caught = {m: [] for m in RM.MISREADINGS}
    for depth in (1, 64, 500):
        for deleted in (False, True):
            for Q in RM.plateau_batch(P):
                ix, terms, pl, ms = RM.plateau_model(P, Q, depth, deleted)
                right = RM.replay(ix, terms, pl.cand, depth, ms).result
                for m in RM.MISREADINGS:
                    if RM.replay(ix, terms, pl.cand, depth, ms, misread=m).result != right:
                        caught[m].append(f"{Q['name']} (depth {depth}{', deleted' if deleted else ''})")
    for m, qs in caught.items():
        print(f"misreading '{m}' changes {len(qs)} (query, depth, deletion) cases: {sorted(set(qs))}")
    for m, qs in caught.items():
        assert qs, m
