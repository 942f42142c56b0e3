"""tests/stage1_model.py pinned to the oracle on the CPU: the model reads the same CSR arrays and term lists and must arrive at the oracle's mode, candidate
count, top-500 set and scores — so that what tests/test_gpu_stage1_edges.py holds the kernels to is the reference's Stage 1 and not the model's own idea of
it.  Also here: the share of rows of the constructed index that lie within the tolerance of a cut, which bounds what that GPU test may excuse."""
import numpy as np
import pytest

from tests import oracle_lib as O
from tests import stage1_model as M
from tools.synth import Synth

DEPTH = 500
NQ, QSEED = 150, 17
SKIP_CAP = 0.10


@pytest.fixture(scope="module")
def oracle():
    s = Synth(2, docs=20000)
    arena, offs = s.docs()
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    return s, o


def test_model_equals_the_oracle(oracle):
    """Every query: mode, candidate count, top-500 set (except among documents whose model score lies within the tolerance of the cut) and every common
    score within (10 + n_terms) * 2^-24 of the float64 model.  A query whose candidates depend on the order the BCL's unstable sort gives terms of equal
    idf (Plan.ambiguous) is skipped, as is one with a fuzzy virtual term (its doc set is not in the exported arrays); at most 10 % may be."""
    s, o = oracle
    ex = o.export_index()
    po, pd, pw = ex["post_off"], ex["post_doc"], ex["post_w"]
    ix = M.Index(ex["doc_len"], np.float32(o.avgdl))
    assert ix.N == o.num_docs
    qa, qo = s.queries(NQ, qseed=QSEED, fuzz=0.0)
    texts = Synth.texts(qa, qo)
    skipped = checked = excused = 0
    modes = {1: 0, 2: 0, 3: 0}
    worst = 0.0
    for q in texts:
        o.search(q, 10, DEPTH)
        tid, df, idf, _ = o.last_terms()
        st = o.last_stats()
        ok, osc = o.last_stage1()
        if len(tid) == 0:
            assert len(ok) == 0
            continue
        if (tid < 0).any():
            skipped += 1
            continue
        assert (np.diff(tid) > 0).all()                                   # Bm25Scorer order: ascending term id
        terms = [M.Term(pd[int(po[t]):int(po[t + 1])], pw[int(po[t]):int(po[t + 1])], i, d) for t, d, i in zip(tid.tolist(), df.tolist(), idf.tolist())]
        for t, d in zip(terms, df.tolist()):
            assert len(t.docs) == d and abs(t.idf - M.idf32(ix.N, d)) <= np.spacing(t.idf)      # the model's fp32 idf is the oracle's, to the ulp two logf may differ by
        ql = q.lower()
        sets = [o.prefix_docset(ql[:n]) for n in range(min(len(ql), 3), 0, -1)]
        P = M.plan(ix, terms, DEPTH, sets)
        if P.ambiguous:
            skipped += 1
            continue
        checked += 1
        modes[P.mode] += 1
        assert P.mode == st["mode"], (q, P.mode, st)
        assert int(P.cand.sum()) == st["candidates"], (q, int(P.cand.sum()), st)
        rw = M.rows(ix, P, M.scores(ix, terms))
        got = dict(zip(ok.tolist(), osc.tolist()))                        # internal id == DocumentKey here
        excused += M.check_rows(got, rw, DEPTH, len(terms), q)
        worst = max([worst] + [abs(float(v) - rw[d]) / rw[d] / M.tolerance(len(terms)) for d, v in got.items()])
    share = skipped / len(texts)
    print(f"stage-1 model vs oracle: {checked} queries checked, modes {modes}, {skipped} skipped ({100 * share:.1f} %), {excused} rows excused at a cut, "
          f"worst score error {worst:.2f} of the tolerance")
    assert share <= SKIP_CAP, (skipped, len(texts))
    assert all(modes.values()), modes                                      # prefix, disjunctive and AND queries were all among them


def test_model_tolerance_has_room_for_fp32():
    """An fp32 numpy restatement of the same arithmetic stays below 13 * 2^-24 of the float64 model at 128 terms: the bound (138 * 2^-24 there) has room for
    FMA contraction, none for a lost or doubled posting (one posting of 128 is 1 / 128 of the score)."""
    rng = np.random.default_rng(5)
    f32 = np.float32
    n, T = 4096, 128
    dl = (20 + 200 * rng.random(n)).astype(f32); avgdl = f32(dl.mean(dtype=f32))
    ix = M.Index(dl, avgdl)
    terms = [M.Term(np.arange(n), rng.integers(1, 256, n), M.idf32(100000, int(rng.integers(1, 50000)))) for _ in range(T)]
    want = M.scores(ix, terms)
    norm = f32(1.2) * (f32(0.25) + (f32(0.75) / avgdl) * dl)
    acc = np.zeros(n, f32)
    for t in terms:
        tf = t.tf.astype(f32)
        acc = acc + t.idf * ((tf * f32(f32(1.2) + f32(1.0))) / (tf + norm) + f32(1))
    assert acc.dtype == f32 and norm.dtype == f32
    rel = np.abs(acc.astype(np.float64) - want) / want
    print(f"fp32 restatement at {T} terms: worst error {rel.max() * 2 ** 24:.2f} * 2^-24")
    assert rel.max() <= 13 * 2.0 ** -24 and M.tolerance(T) * want.min() < float(min(t.idf for t in terms))


@pytest.mark.parametrize("R", M.WIDTHS)
def test_constructed_index_keeps_the_cut_excuses_small(R):
    """The constructed index of tests/test_gpu_stage1_edges.py on the model alone: at every width and for every query, with and without the deletions, the rows
    within the tolerance of the cut are well under the 2 % that test may excuse, and no query depends on the order of equal idfs."""
    E = M.EdgeIndex(R)
    assert E.N == 4 * R + R // 2 + 3 and set(np.unique(E.post_w).tolist()) == set(range(1, 256))      # every tf byte from 1 to 255 occurs
    assert (E.doc_len > 0).all() and len(np.unique(E.doc_len)) > 0.99 * E.N
    assert R != 16384 or 65535 in E.lists[0].tolist()
    worst = 0.0
    for deleted in (False, True):
        for Q in M.edge_batch(E, 2):
            terms, P, sc, counts, rw = M.edge_model(E, Q, deleted)
            assert not P.ambiguous, Q["name"]
            if len(rw) > M.EDGE_DEPTH:
                worst = max(worst, M.near_cut(rw, M.EDGE_DEPTH, M.tolerance(len(terms))) / M.EDGE_DEPTH)
    print(f"R = {R}: at most {100 * worst:.2f} % of a query's rows lie within the tolerance of its cut")
    assert worst <= 0.015
