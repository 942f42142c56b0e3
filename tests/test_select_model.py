"""tests/select_model.py on the CPU: cut() against an independent statement of itself, the rule read from class counts against stage1_model.plan's candidates, every
named query of the constructed batch on the path it was built for (so that an edit of the fixture cannot quietly lose a path), the band-edge rows at 0 and -1 ulp, and
four misreadings of the cut each told from the right reading by at least one named query.  tests/test_gpu_select_cuts.py holds the kernels to this model."""
import numpy as np
import pytest

from tests import replay_model as RM
from tests import select_model as SM
from tests import stage1_model as M

f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def index():
    return SM.SelectIndex()


@pytest.fixture(scope="module")
def models(index):
    """deleted -> [(query, Sel)] of the named queries."""
    return {deleted: [(Q, index.select(Q, deleted)) for Q in SM.select_queries()] for deleted in (False, True)}


def test_the_index_is_the_size_the_kernels_need(index):
    assert index.N == 70001 and index.N > 65536
    qs = SM.select_queries()
    assert {1, 2, 63, 64, 65, 500, 1024} <= {Q["depth"] for Q in qs}
    assert max(Q["depth"] for Q in qs) <= SM.MAX_DEPTH
    assert len({Q["name"] for Q in qs}) == len(qs)
    for level, n in enumerate(SM.BATCH_SIZES):
        b = SM.select_batch(level)
        assert len(b) == n and [Q["name"] for Q in b[:len(qs)]] == [Q["name"] for Q in qs]
        for Q in b:                                        # terms in ascending term id: the scorer's order
            ids = [index.id[t] for t, _ in Q["terms"]]
            assert ids == sorted(ids) and len(set(ids)) == len(ids)
    assert SM.BATCH_SIZES == (63, 64, 65, 100)
    assert SM.batch_bound(index, SM.select_batch(3)) >= 4 * 16384      # the sweeps are launched at INFX_SEL_GIANT_MIN = 16384 (not at 20000: 80 000 > N)
    assert (index.gone[:-1] < index.gone[1:]).all() and index.gone[-1] < index.N


def test_cut_agrees_with_a_python_sort(models):
    for deleted, per in models.items():
        for Q, S in per:
            C = S.cut()
            sc = S.bits.view(f32).astype(np.float64)
            rows = sorted(zip((-sc).tolist(), S.docs.tolist()))
            want = rows[:Q["depth"]]
            assert C.hits == len(want) == len(C.docs), Q["name"]
            assert [d for _, d in want] == C.docs.tolist(), Q["name"]
            assert [int(f32(-s).view(u32)) for s, _ in want] == C.bits.tolist(), Q["name"]
            nxt = -rows[Q["depth"]][0] if len(rows) > Q["depth"] else 0.0
            assert float(C.next) == nxt, Q["name"]
            if nxt > 0:
                c = f32(-want[-1][0])
                assert C.flagged == bool(f32(nxt) >= f32(c * f32(f32(1) - f32(1e-5)))), Q["name"]
                assert C.why == (None if not C.flagged else 0 if f32(nxt) == c else 1), Q["name"]
            else:
                assert not C.flagged and C.why is None, Q["name"]
            assert (C.why if C.flagged else None) == Q["flag"] or (deleted and Q["name"] in FLAG_CHANGES_WHEN_DELETED), (Q["name"], C.flagged, C.why)


FLAG_CHANGES_WHEN_DELETED = ()


def test_rule_from_class_counts_accepts_the_plans_candidates(index, models):
    for deleted, per in models.items():
        for Q, S in per:
            docs, sc = RM.first_pass(S.ix, S.terms, S.plan.cand)
            want = docs[(sc > 0) & ~S.ix.deleted[docs]]
            assert np.array_equal(np.sort(S.docs), want), (Q["name"], len(S.docs), len(want))
            assert np.array_equal(S.counts, M.class_counts(S.ix, S.terms, S.plan, M.scores(S.ix, S.terms))), Q["name"]
            if Q["mode"] == M.MODE_DISJ:
                assert S.rule.total == int(S.counts[:S.rule.cutoff + 1].sum()) + 128
    kinds = {Q["mode"] for Q, _ in models[False]}
    assert kinds == {M.MODE_DISJ, M.MODE_AND, M.MODE_PREFIX}
    assert any(S.rule.cutoff == 0 and S.plan.df_s1 > 1 for _, S in models[False]), "a cutoff rank that rejects rows"
    assert any(S.rule.mask == 1 for _, S in models[False]), "an AND class mask"


def test_every_named_query_takes_its_path(index, models):
    bound = SM.batch_bound(index, SM.select_batch(3))
    reached, shifts = set(), set()
    for Q, S in models[False]:
        off = SM.path_of(S, False); on = SM.path_of(S, True)
        assert off == (Q["path"], Q["digit"]), (Q["name"], off)
        assert on[0] == Q["path3"], (Q["name"], on)
        swept = SM.path_of(S, True, 64, 64, True, bound)
        assert swept[0] == (Q["swept"] or Q["path3"]), (Q["name"], swept)
        assert SM.path_of(S, True, 64, 63, True, bound) == on and SM.path_of(S, True, 64, 100, False, bound) == on     # no order kernel: no sweeps
        assert SM.path_of(S, True, 20000, 100, True, bound) == on          # 4 * 20000 rows is more than the index holds: the sweeps are not launched
        assert SM.path_of(S, True, 65536, 100, True, bound) == on
        reached |= {off[0], on[0], swept[0]}
        if off[0] in ("radix", "radix after a missed window"):
            shifts |= set(SM._radix(S.docs, S.bits, S.depth, S.rule.total))
    assert reached == set(SM.PATHS)
    assert shifts == {52, 40, 28, 16, 4}                   # (_radix asserts that the pass at shift 0 is never made)
    by_name = {Q["name"]: S for Q, S in models[False]}
    # what the names promise beyond the path
    assert len(by_name["mode 1 2049 rows prefix"].docs) == 2049 and by_name["mode 1 2049 rows prefix"].rule.total == 2049
    assert len(by_name["take-all 2048 rows prefix"].docs) == 2048 and by_name["take-all 2048 rows prefix"].rule.total == SM.SEL_CAP
    assert by_name["take-all 1920 rows disj"].rule.total == SM.SEL_CAP and by_name["mode 1 1921 rows disj"].rule.total == SM.SEL_CAP + 1
    S = by_name["take-all holes and deletions"]
    assert S.arena > len(S.docs) and np.isin(index.gone, S.docs).any()
    S = by_name["mode 1 40000 rows"]
    assert S.arena == 40000 and -(-S.arena // max(SM.PART_MIN, -(-S.arena // SM.PARTS))) == 3        # three partitions of 16 384
    S = by_name["mode 2 first value"]
    assert S.cut().bits[0] == S.origin
    for n in ("plateau one block", "plateau one block depth 1024", "plateau both containers", "plateau below better rows"):
        S = by_name[n]; C = S.cut()
        plateau = int((S.bits == C.bits[-1]).sum())
        assert plateau >= SM.SEL_CAP + 1 + S.depth and C.why == 0, n
    S = by_name["plateau one block"]
    assert len(set((S.docs >> 16).tolist())) == 1
    S = by_name["plateau both containers"]
    assert set((S.docs >> 16).tolist()) == {0, 1}
    S = by_name["plateau below better rows"]
    assert 0 < int((S.bits > S.cut().bits[-1]).sum()) < S.depth and ((S.origin - S.bits.astype(np.int64)) >> SM.FINE).max() == 0      # takeAbove > 0, inside the cut's bin
    S = by_name["second attempt"]
    assert S.origin > int(S.bits.max()) and f32(4) * S.bits.max().view(f32) < np.asarray(S.origin, u32).view(f32)
    S = by_name["rejected giant"]
    assert S.arena >= 20000 and S.rule.total <= SM.SEL_CAP
    rows = [S.arena for _, S in models[False]]
    assert len(rows) - len(set(rows)) >= 3                 # queries of equal row count: the order's tie rule
    # with deletions every query keeps its path but for the counts of rows (the rule's total counts deleted documents too)
    for Q, S in models[True]:
        assert SM.path_of(S, False) == (Q["path"], Q["digit"]), Q["name"]
    assert len(dict((Q["name"], S) for Q, S in models[True])["exactly depth rows"].docs) == SM.EDGE_DEPTH


def test_band_edge_rows_sit_at_zero_and_minus_one_ulp(index, models):
    by_name = {Q["name"]: S for Q, S in models[False]}
    assert 64 <= index.edge_ulps <= 200
    for name, dist, gathered, flag in (("band edge gathered", 0, True, 1), ("band edge not gathered", 0, False, 1), ("band below gathered", -1, True, None),
                                       ("band below not gathered", -1, False, None), ("band equal", None, True, 0)):
        S = by_name[name]; C = S.cut()
        c = C.bits[-1:].view(f32)[0]
        nb = int(SM.bits(C.next))
        if dist is None:
            assert nb == int(C.bits[-1])
        else:
            assert nb - int(SM.bits(SM.band_edge(c))) == dist, name
        same_bin = ((S.origin - nb) >> SM.FINE) == ((S.origin - int(C.bits[-1])) >> SM.FINE)
        assert same_bin == gathered, name
        assert (C.why if C.flagged else None) == flag, name
        assert C.hits == S.depth == SM.EDGE_DEPTH
    for deleted in (False, True):
        S = dict((Q["name"], S) for Q, S in models[deleted])["exactly depth rows"]
        C = S.cut()
        assert (float(C.next) == 0) == deleted and not C.flagged


@pytest.mark.parametrize("misread", SM.MISREADINGS)
def test_the_batch_tells_a_misreading_from_the_right_one(models, misread):
    told = []
    for Q, S in models[False]:
        a, b = S.cut(), S.cut(misread)
        same = (a.hits == b.hits and np.array_equal(a.docs, b.docs) and np.array_equal(a.bits, b.bits) and SM.bits(a.next) == SM.bits(b.next)
                and a.flagged == b.flagged and a.why == b.why)
        if not same:
            told.append(Q["name"])
    assert told, misread
    want = {SM.MISREADINGS[0]: "plateau one block", SM.MISREADINGS[1]: "band edge gathered", SM.MISREADINGS[2]: "band edge not gathered",
            SM.MISREADINGS[3]: "second attempt"}[misread]
    assert want in told, (misread, told)


def test_tiny_batches(index):
    T = SM.TinyIndex()
    qs = SM.tiny_batch(4097)
    assert len(qs) == SM.ORDER_MAX + 1
    for Q in qs[:50]:
        S = T.select(Q)
        assert len(S.docs) == 1 and SM.path_of(S, True, 64, 4096, True, 1) == ("take-all", None)
