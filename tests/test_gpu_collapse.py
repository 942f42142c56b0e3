"""Query.collapse_by on the GPU: at most collapse_keep ranked rows per value of a field (k_finalize's window + k_collapse).

The contract: for a query Q with collapse_by, let Q0 be Q without collapsing, filter, facets, boosts and sort_by and with max_number_of_records_to_return =
coverage_depth; L = Q0's rows.  A row of L is kept when fewer than collapse_keep earlier rows of L have its group (the dictionary code of its document in the
column); Q returns the first max_number_of_records_to_return kept rows, Q0's flags, and the post-processing then works on those rows.

The expected answer is a fold in plain Python (fold below) over L and the columns the test itself set; it never comes from the collapsing code.  L is the
engine's own answer to Q0 — a query without collapse_by, which takes the path it took before this option existed — except in the anchor test, where L is the
oracle's.  Keys are unique in these corpora (the key is the document's index), so a row's document is its key's.  Filter, boosts and sort-by on the folded
rows are tests/test_gpu_boost_sort.py's restatement (the oracle's filter VM, tests/bcl_sort.py), facets tests/browse_model.py's.  Every comparison is exact:
keys, score bits, tiebreakers, flags, group_values, group_sizes, total_groups, total_ranked."""
import dataclasses
import os
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength, CoverageSetup
from infidex_amd.engine import Session
from tests import oracle_lib as O
from tests.browse_model import BrowseModel, facet_text
from tests.parity_classify import score_matches, ulp, final_blend_slack, FINAL_SCORE_TOL, stage2_scored, bits
from tests.test_gpu_boost_sort import Fixture, columns, rows_of, assert_rows
from tests.test_gpu_list_documents import D
from tests.test_gpu_post_rows import DOCS as PLATEAU_DOCS, TEXTS as PLATEAU_TEXTS
from tools.synth import Synth

pytestmark = pytest.mark.gpu

KEEPS = [1, 2, 3, 16]
NO_TRUNCATE = CoverageSetup(truncate=False)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def group_id(v):
    """What makes two values one group: the dictionary's rule — a double by its bit pattern (-0.0, 0.0 and every NaN payload apart), anything else by its text."""
    if isinstance(v, (float, np.floating)):
        return struct.pack("<d", float(v))
    return facet_text(v)


def fold(L, vals, keep, mr):
    """L: [(key, score, tie)] in rank order, vals: the collapse column by document.  (rows returned, their group texts, their group sizes, groups, len(L))"""
    sizes, seen, rows = {}, {}, []
    for k, _, _ in L:
        g = group_id(vals[k]); sizes[g] = sizes.get(g, 0) + 1
    for r in L:
        g = group_id(vals[r[0]])
        if seen.get(g, 0) < keep and len(rows) < mr:
            rows.append(r)
        seen[g] = seen.get(g, 0) + 1
    return rows, [facet_text(vals[k]) for k, _, _ in rows], [sizes[group_id(vals[k])] for k, _, _ in rows], len(sizes), len(L)


def q0_of(q):
    return dataclasses.replace(q, collapse_by=None, collapse_keep=1, filter=None, enable_facets=False, enable_boost=False, boosts=None, sort_by=None,
                               max_number_of_records_to_return=int(q.coverage_depth))


def flags_of(r):
    return (r.unsupported, r.used_coverage, r.stage1_fallback, r.skipped_candidates)


def once(e, qs):
    s = Session(e)
    try:
        return s.search_queries(qs), s.last_collapse_stats()
    finally:
        s.close()


def assert_collapsed(r, L, l_flags, vals, q, ctx):
    """r: the engine's answer to q (collapse_by, no post-processing) against the fold of L"""
    rows, gv, gs, groups, ranked = fold(L, vals, q.collapse_keep, q.max_number_of_records_to_return)
    assert r.error is None, (ctx, r.error)
    assert_rows(rows_of(r), rows, ctx)
    assert flags_of(r) == l_flags, ctx
    assert (r.group_values, r.group_sizes, r.total_groups, r.total_ranked) == (gv, gs, groups, ranked), (ctx, r.group_values[:6], gv[:6], r.group_sizes[:6], gs[:6],
                                                                                                         r.total_groups, groups, r.total_ranked, ranked)


def same_answer(a, b, ctx):
    assert a.error == b.error, (ctx, a.error, b.error)
    assert_rows(rows_of(a), rows_of(b), ctx)
    assert flags_of(a) == flags_of(b) and a.facets == b.facets and a.total_in_filter == b.total_in_filter, ctx
    assert (a.group_values, a.group_sizes, a.total_groups, a.total_ranked) == (b.group_values, b.group_sizes, b.total_groups, b.total_ranked), ctx


# ---- every list length, column kind, keep and budget --------------------------------------------------------------------------------------------------
N_SMALL = 1100
SPECIAL = np.array([0x8000000000000000, 0x0000000000000000, 0x7FF8000000000000, 0x7FF8000000000001, 0x3FF8000000000000, 0x4004000000000000], np.uint64).view(np.float64)


def small_columns(n):
    k = np.arange(n)
    year, rating, genre = columns(n)
    return {"one": (np.full(n, 7, np.int64), False), "uniq": ((k * 3 - 50).astype(np.int64), False), "two": ((k % 2).astype(np.int64), True),
            "ten": ((k % 10).astype(np.int64), True), "giant": (np.where(k < (6 * n) // 10, -1, k).astype(np.int64), False),
            "word": (["w%d" % (i % 7) for i in k], True), "dbl": (SPECIAL[k % len(SPECIAL)].copy(), False),
            "year": (year, True), "rating": (rating, False), "genre": (genre, True)}


COLLAPSE_COLS = ["one", "uniq", "two", "ten", "giant", "word", "dbl"]


def small_engine(n, **kw):
    e = SearchEngine.create_default(device=0, **kw)
    e.index_documents([Document(k, "alpha %s lot %d" % (["red", "green", "golden"][k % 3], k)) for k in range(n)])
    cols = small_columns(n)
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    return e, cols


@pytest.fixture(scope="module")
def small():
    return small_engine(N_SMALL), small_engine(N_SMALL, max_depth=1024)


def test_the_special_doubles_are_four_groups():
    v = SPECIAL
    assert v[0] == 0 and np.signbit(v[0]) and v[1] == 0 and not np.signbit(v[1]) and np.isnan(v[2]) and np.isnan(v[3])
    assert len({group_id(x) for x in v}) == 6
    L = [(k, 1.0, 0) for k in range(12)]
    assert fold(L, v[np.arange(12) % 6], 1, 12)[3] == 6 and fold(L, v[np.arange(12) % 6], 1, 12)[2] == [2] * 6


@pytest.mark.parametrize("coverage", [True, False])
@pytest.mark.parametrize("depth", [1, 2, 63, 64, 65, 255, 256, 257, 500, 1024])
def test_every_length_column_keep_and_budget(small, depth, coverage):
    """Every document holds the query word.  Without coverage L is the Stage-1 list: exactly `depth` rows, the lengths the kernel's paths turn on.  With
    coverage and truncate=False L is what Stage 2 leaves of `depth` scored rows once the two rows of a document (its WordMatcher row and its Stage-1 row) are
    consolidated into one: measured 1 row at depth 2 — not `depth` rows; whatever its length, it is folded as it stands."""
    (e, cols), (e1024, _) = small
    eng = e1024 if depth > 500 else e
    l_res = eng.search_queries([Query("alpha", depth, depth, coverage, coverage_setup=NO_TRUNCATE)])[0]
    L = rows_of(l_res)
    print("depth %d coverage %s: L has %d rows" % (depth, coverage, len(L)))
    assert 1 <= len(L) <= depth and (coverage or len(L) == depth), (depth, coverage, len(L))
    ten = rows_of(eng.search_queries([Query("alpha", 10, depth, coverage)])[0])
    assert ten == L[:len(ten)] and len(ten) >= 1, (depth, len(ten))                  # L extends the ten-row answer of the default setup
    qs = [Query("alpha", mr, depth, coverage, coverage_setup=NO_TRUNCATE, collapse_by=c, collapse_keep=keep)
          for c in COLLAPSE_COLS for keep in KEEPS for mr in sorted({1, 10, 64, depth})]
    s = Session(eng)
    res = s.search_queries(qs)
    assert s.last_collapse_stats() == (len(qs), 1)
    s.close()
    for q, r in zip(qs, res):
        assert_collapsed(r, L, flags_of(l_res), cols[q.collapse_by][0], q, (depth, coverage, q.collapse_by, q.collapse_keep, q.max_number_of_records_to_return))
    by = {(q.collapse_by, q.collapse_keep, q.max_number_of_records_to_return): r for q, r in zip(qs, res)}
    assert len(by[("one", 1, depth)].records) == 1 and by[("one", 1, depth)].group_sizes == [len(L)]
    assert rows_of(by[("uniq", 1, depth)]) == L and by[("uniq", 1, depth)].total_groups == len(L)


def test_lists_shorter_than_the_depth_and_empty_lists(small):
    (e, cols), _ = small
    e3, cols3 = small_engine(3)
    l_res = e3.search_queries([Query("alpha", 500, 500, True, coverage_setup=NO_TRUNCATE)])[0]
    L = rows_of(l_res)
    assert 1 <= len(L) <= 3
    qs = [Query("alpha", mr, 500, True, coverage_setup=NO_TRUNCATE, collapse_by=c, collapse_keep=keep) for c in COLLAPSE_COLS for keep in (1, 2, 16) for mr in (1, 10)]
    for q, r in zip(qs, e3.search_queries(qs)):
        assert_collapsed(r, L, flags_of(l_res), cols3[q.collapse_by][0], q, (q.collapse_by, q.collapse_keep, q.max_number_of_records_to_return))
    # a text that matches nothing, and an empty text without facets: empty lists, no error
    res = e.search_queries([Query("zzzzqqqqxxxx", 10, 500, True, collapse_by="ten", collapse_keep=2), Query("", 10, 500, True, collapse_by="ten"), Query("alpha", 3, collapse_by="ten")])
    for r in res[:2]:
        assert r.error is None and r.records == [] and (r.group_values, r.group_sizes, r.total_groups, r.total_ranked) == ([], [], 0, 0), r
    assert len(res[2].records) == 3 and e.last_collapse_stats() == (3, 1)
    # SearchEngine.search routes a collapsing query to search_queries
    one = e.search(Query("alpha", 3, collapse_by="ten"))
    same_answer(one, res[2], "search")


# ---- truncation is decided on the uncollapsed list ------------------------------------------------------------------------------------------------------
def test_the_row_at_the_truncation_index_may_be_collapsed_away():
    """The default CoverageSetup on the plateau corpus: L ends at the truncation index.  The column — the colour in the document's text, five groups — is chosen
    from the oracle's lists alone: with one row kept per group the last row of every list, the row AT the truncation index, is collapsed away."""
    n = len(PLATEAU_DOCS)
    o = O.OracleEngine.create_default(); o.index(PLATEAU_DOCS)
    vals = (np.arange(n) % 5).astype(np.int64) + 40
    for t in PLATEAU_TEXTS:                                                          # the condition, before the engine is looked at
        w = o.search(t, 500, 500, True)["keys"]
        assert len(w) > 5 and any(vals[k] == vals[w[-1]] for k in w[:-1]), t
    e = SearchEngine.create_default(device=0); e.index_documents([Document(k, t) for k, t in PLATEAU_DOCS])
    e.set_column("fam", vals, facetable=False)
    for t in PLATEAU_TEXTS:
        l_res = e.search_queries([Query(t, 500, 500, True)])[0]                      # truncated where the default setup truncates
        L = rows_of(l_res)
        assert len(L) > 5 and any(vals[k] == vals[L[-1][0]] for k, _, _ in L[:-1]), t
        for keep, mr in ((1, 500), (1, 3), (2, 500), (16, 64)):
            q = Query(t, mr, 500, True, collapse_by="fam", collapse_keep=keep)
            r = e.search_queries([q])[0]
            assert_collapsed(r, L, flags_of(l_res), vals, q, (t, keep, mr))
            assert keep > 2 or L[-1][0] not in [x.document_id for x in r.records]


# ---- anchored to the reference: L is the oracle's ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anchor():
    s = Synth(2, docs=40000)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    year, rating, genre = columns(40000)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    qa, qo = s.queries(ANCHOR_QUERIES, qseed=43, fuzz=0.3)
    return e, o, {"year": year, "genre": genre}, Synth.texts(qa, qo)


ANCHOR_QUERIES, ANCHOR_DEPTH = 240, 100


def swappable(a, b, coverage):
    """parity_classify's order rule from the oracle's side: two neighbours may come back swapped only when their oracle scores are not bit-equal (rows that carry
    the oracle's bits are in the total order (score, tiebreaker, key)) and lie within the allowance of score_matches of each other"""
    a, b = float(np.float32(a)), float(np.float32(b))
    lo = min(a, b)
    return bits(a) != bits(b) and abs(a - b) <= min(ulp(lo) + final_blend_slack(lo) if coverage else 2e-6 * 32 * max(abs(lo), 1e-9), FINAL_SCORE_TOL)


def anchor_cases(o, cols, texts):
    """The queries whose oracle answer is unambiguous: no swappable pair of neighbours up to and including the last row the fold returns (the whole list where the
    fold returns fewer than asked) — what lies behind that row only counts into the sizes, whatever its order.  (indices, queries, [(oracle result, fold)])"""
    picked, qs, want = [], [], []
    for i, t in enumerate(texts):
        w = o.search(t, ANCHOR_DEPTH, ANCHOR_DEPTH, True)
        if len(w["keys"]) < 5:
            continue
        w["stage2_scored"] = stage2_scored(o, w)
        name = ("genre", "year")[i % 2]
        q = Query(t, 10, ANCHOR_DEPTH, True, collapse_by=name, collapse_keep=1 + (i // 2) % 2)
        L = list(zip(w["keys"], [float(x) for x in w["scores"]], w["ties"].tolist()))
        f = fold(L, cols[name], q.collapse_keep, 10)
        last = w["keys"].index(f[0][-1][0]) if len(f[0]) == 10 else len(L) - 1
        sc = w["scores"]
        if any(swappable(sc[j], sc[j + 1], w["stage2_scored"]) for j in range(min(last + 1, len(L) - 1))):
            continue
        picked.append(i); qs.append(q); want.append((w, f))
    return picked, qs, want


def test_the_fold_of_the_oracles_list(anchor):
    e, o, cols, texts = anchor
    picked, qs, want = anchor_cases(o, cols, texts)
    assert len(picked) >= 20, len(picked)
    assert sum(1 for w, f in want if [r[0] for r in f[0]] != w["keys"][:10]) >= 5     # the fold changes rows
    for q, r, (w, (rows, gv, gs, groups, ranked)) in zip(qs, e.search_queries(qs), want):
        ctx = (q.text, q.collapse_by, q.collapse_keep)
        assert r.error is None, (ctx, r.error)
        assert [x.document_id for x in r.records] == [k for k, _, _ in rows], (ctx, [x.document_id for x in r.records], [k for k, _, _ in rows])
        assert [x.tiebreaker for x in r.records] == [t for _, _, t in rows], ctx
        for x, (k, sc, _) in zip(r.records, rows):
            score_matches(x.score, sc, w["stage2_scored"], what=(ctx, k))
        assert (r.group_values, r.group_sizes, r.total_groups, r.total_ranked) == (gv, gs, groups, ranked), (ctx, r.group_sizes, gs, r.total_groups, groups, r.total_ranked, ranked)


# ---- a mixed batch ----------------------------------------------------------------------------------------------------------------------------------
MIX_FIELDS = ["ten", "shop", "genre", "wide", "uniq"]
MIX_WEIGHTS = [0.3, 0.25, 0.25, 0.1, 0.1]        # (a list of a few hundred rows rarely holds a value of `wide` twice, never one of `uniq`: those fold nothing away)
MIX_PRE = ["year >= 1980", "genre != 'Horror' AND rating > 2.0"]
MIX_FILTERS = ["year >= 1960 AND genre != 'Horror'", "rating > 5.5 AND rating < 8.5"]
MIX_BOOSTS = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low)]
# The seed was chosen with the oracle alone, on the CPU (its lists of the same queries, the pre-filters as deletions): 50 of the 100 queries collapse, all five
# fields occur, the fold changes the rows of 34 of them, 31 fill their max_number_of_records_to_return and 19 do not.  The test asserts the three conditions
# again, on the lists it folds, before it compares.
MIX_SEED = 16


def mixed_queries(texts, seed=MIX_SEED, n=100):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kw = {}
        if rng.random() < 0.5:
            kw.update(collapse_by=MIX_FIELDS[int(rng.choice(len(MIX_FIELDS), p=MIX_WEIGHTS))], collapse_keep=int(rng.integers(1, 4)))
        if rng.random() < 0.2:
            kw["pre_filter"] = MIX_PRE[int(rng.integers(len(MIX_PRE)))]
        if rng.random() < 0.3:
            kw["filter"] = MIX_FILTERS[int(rng.integers(len(MIX_FILTERS)))]
        if rng.random() < 0.3:
            kw["enable_facets"] = True
        if rng.random() < 0.25:
            kw.update(enable_boost=True, boosts=MIX_BOOSTS)
        if rng.random() < 0.3:
            kw.update(sort_by=["year", "rating", "genre"][int(rng.integers(3))], sort_ascending=bool(rng.random() < 0.5))
        out.append(Query(texts[i % len(texts)], int(rng.choice([5, 10, 20, 64])), 500, bool(rng.random() < 0.8), **kw))
    return out


@pytest.fixture(scope="module")
def mixed():
    syn = Synth(2, docs=D)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, syn.field_weights)
    rng = np.random.default_rng(23)                                                  # (the columns of tests/test_gpu_list_groups.py)
    year, rating, genre = columns(D)
    shop = rng.integers(0, 99, D).astype(np.int64); shop[D - 1] = 99
    ten = ["c%d" % v for v in rng.integers(0, 10, D)]
    wide = rng.permutation(np.arange(D, dtype=np.int64) % 55000 + 100000)
    uniq = rng.permutation(np.arange(D, dtype=np.int64)) * 3 - 5000
    cols = {"shop": (shop, False), "year": (year, True), "rating": (rating, False), "genre": (genre, True), "ten": (ten, True), "wide": (wide, False), "uniq": (uniq, False)}
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    qa, qo = syn.queries(60, qseed=43, fuzz=0.3)
    return e, cols, BrowseModel(cols), Fixture(e, None, (year, rating, genre)), Synth.texts(qa, qo)


def expected_mixed(q, L, l_res, cols, model, F):
    rows, _, _, groups, ranked = fold(L, cols[q.collapse_by][0], q.collapse_keep, q.max_number_of_records_to_return)
    kept = [r for r in rows if q.filter is None or F.holds(q.filter, r[0])]
    final = F.expected(kept, q.enable_boost, q.boosts, q.sort_by, q.sort_ascending)
    sizes = {}
    for k, _, _ in L:
        g = group_id(cols[q.collapse_by][0][k]); sizes[g] = sizes.get(g, 0) + 1
    return rows, kept, final, [facet_text(cols[q.collapse_by][0][k]) for k, _, _ in final], [sizes[group_id(cols[q.collapse_by][0][k])] for k, _, _ in final], groups, ranked


def check_mixed(q, r, L, l_res, cols, model, F, ctx):
    rows, kept, final, gv, gs, groups, ranked = expected_mixed(q, L, l_res, cols, model, F)
    assert r.error is None, (ctx, r.error)
    assert_rows(rows_of(r), final, ctx)
    assert flags_of(r) == flags_of(l_res), ctx
    assert (r.group_values, r.group_sizes, r.total_groups, r.total_ranked) == (gv, gs, groups, ranked), (ctx, r.group_sizes, gs, r.total_groups, groups, r.total_ranked, ranked)
    if q.enable_facets:
        assert (r.facets or {}) == model.row_facets([k for k, _, _ in kept]), ctx


def test_mixed_batch(mixed):
    e, cols, model, F, texts = mixed
    qs = mixed_queries(texts)
    clp = [i for i, q in enumerate(qs) if q.collapse_by is not None]
    assert 35 <= len(clp) <= 65 and {qs[i].collapse_by for i in clp} == set(MIX_FIELDS)
    l_res, stats = once(e, [q0_of(qs[i]) for i in clp])
    assert stats == (0, 0)
    Ls = {i: rows_of(r) for i, r in zip(clp, l_res)}
    lr = dict(zip(clp, l_res))
    # the conditions the seed was chosen for, from the fold alone
    folded = {i: fold(Ls[i], cols[qs[i].collapse_by][0], qs[i].collapse_keep, qs[i].max_number_of_records_to_return)[0] for i in clp}
    changed = sum(1 for i in clp if folded[i] != Ls[i][:qs[i].max_number_of_records_to_return])
    full = sum(1 for i in clp if len(folded[i]) == qs[i].max_number_of_records_to_return)
    print("mixed batch: %d collapsing, %d changed, %d full, %d not full" % (len(clp), changed, full, len(clp) - full))
    assert 2 * changed >= len(clp) and full >= 10 and len(clp) - full >= 5, (len(clp), changed, full)
    s = Session(e)
    res = s.search_queries(qs)
    assert s.last_collapse_stats() == (len(clp), 1)
    for i in clp:
        check_mixed(qs[i], res[i], Ls[i], lr[i], cols, model, F, (i, qs[i]))
        alone, st = once(e, [qs[i]])
        assert st == (1, 1)
        same_answer(res[i], alone[0], (i, "alone"))
    # the others: the bytes of the same batch with every collapse_by removed
    stripped, st = once(e, [dataclasses.replace(q, collapse_by=None, collapse_keep=1) for q in qs])
    assert st == (0, 0)
    for i, (r, w) in enumerate(zip(res, stripped)):
        if i not in clp:
            same_answer(r, w, (i, "stripped"))
            assert r.group_values is None and r.total_ranked is None
    # determinism: twice on one session, four sessions on four threads
    again = s.search_queries(qs)
    for i, (a, b) in enumerate(zip(again, res)):
        same_answer(a, b, (i, "repeat"))
    s.close()
    out, err = [None] * 4, []

    def run(k):
        try:
            out[k] = once(e, qs)[0]
        except Exception as x:                                                      # pragma: no cover
            err.append(x)
    th = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k in range(4):
        for i, (a, b) in enumerate(zip(out[k], res)):
            same_answer(a, b, (k, i, "thread"))


# ---- alignment after the post-processing ------------------------------------------------------------------------------------------------------------
def test_group_figures_follow_the_rows_through_filter_and_sort(small):
    (e, cols), _ = small
    model = BrowseModel(cols); F = Fixture(e, None, (cols["year"][0], cols["rating"][0], cols["genre"][0]))
    base = Query("alpha", 64, 500, True, coverage_setup=NO_TRUNCATE)
    l_res = e.search_queries([q0_of(base)])[0]
    L = rows_of(l_res)
    qs = [dataclasses.replace(base, collapse_by=c, collapse_keep=keep, filter="year >= 1975 AND genre != 'Horror'", sort_by=sb, sort_ascending=asc, enable_facets=True)
          for c in ("ten", "word", "dbl", "giant") for keep in (1, 3) for sb, asc in (("rating", True), ("genre", False), (None, False))]
    res = e.search_queries(qs)
    dropped = reordered = 0
    for q, r in zip(qs, res):
        check_mixed(q, r, L, l_res, cols, model, F, (q.collapse_by, q.collapse_keep, q.sort_by))
        rows, kept, final = expected_mixed(q, L, l_res, cols, model, F)[:3]
        dropped += int(len(kept) < len(rows)); reordered += int(final != kept)
        vals = cols[q.collapse_by][0]
        for x, gv, gs in zip(r.records, r.group_values, r.group_sizes):              # row by row: the group of THIS row, its size in L
            assert gv == facet_text(vals[x.document_id]) and gs == sum(1 for k, _, _ in L if group_id(vals[k]) == group_id(vals[x.document_id]))
    assert dropped >= len(qs) // 2 and reordered >= len(qs) // 3


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refused_queries_leave_their_neighbours_alone(small):
    (e, cols), _ = small
    good = [Query("alpha", 10, collapse_by="ten", collapse_keep=2), Query("alpha lot 7", 5), Query("golden", 20, collapse_by="word"), Query("red alpha", 10, filter="year >= 1980")]
    bad = [Query("alpha", 10, collapse_by="nosuch"), Query("alpha", 10, collapse_by="ten", collapse_keep=0), Query("alpha", 10, collapse_by="ten", collapse_keep=17),
           Query("", 10, enable_facets=True, collapse_by="ten")]
    pos = [0, 2, 5, 7]
    mix = list(good)
    for p, b in zip(pos, bad):
        mix.insert(p, b)
    s = Session(e)
    res = s.search_queries(mix)
    assert s.last_collapse_stats() == (2, 1)
    s.close()
    want, _ = once(e, good)
    for r, w in zip([r for i, r in enumerate(res) if i not in pos], want):
        same_answer(r, w, "neighbour")
    for p in pos:
        assert res[p].records == [] and res[p].error and res[p].group_values is None and res[p].total_groups is None, (p, res[p])
    assert "nosuch" in res[0].error and "collapse_keep" in res[2].error and "collapse_keep" in res[5].error and "browse" in res[7].error
    # a batch of another size fails and clears the requests
    from infidex_amd.engine import _install_collapse, pack_texts
    s = Session(e)
    _install_collapse(e, s.h, [good[0]] * 3)
    with pytest.raises(Exception):
        s.search_packed(*pack_texts(["alpha", "golden"]), 10, 500, True)
    k2 = s.search_packed(*pack_texts(["alpha", "golden", "red"]), 10, 500, True)
    plain = e.search_batch(["alpha", "golden", "red"], 10)
    for i in range(3):
        assert [int(k) for k in k2[0][i, :int(k2[3][i])]] == [x.document_id for x in plain[i].records]
    assert s.last_collapse_stats() == (0, 0)
    s.close()


def test_shards_refuse_collapse_by():
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_search_queries
    docs = [Document(k, "alpha bravo %d" % k) for k in range(40)]
    year = np.arange(40, dtype=np.int64) // 4 + 1980
    engs = [create_sharded_engine(r, 2, 0) for r in range(2)]
    for x in engs:
        x.index_documents(docs); x.set_column("year", year, facetable=True)
    qs = [Query("alpha", 10), Query("alpha", 10, collapse_by="year"), Query("bravo 7", 5)]
    got = simulate_search_queries([ShardSession(x) for x in engs], qs)
    assert got[1].records == [] and got[1].error and "shard" in got[1].error and got[1].group_values is None
    u = SearchEngine.create_default(device=0); u.index_documents(docs)
    for r, w in zip((got[0], got[2]), u.search_queries([qs[0], qs[2]])):
        assert r.error is None and w.error is None
        assert_rows(rows_of(r), rows_of(w), "shard neighbour")


def test_host_phases_refuse_collapse_by():
    script = r'''
import numpy as np
from infidex_amd import SearchEngine, Document, Query
e = SearchEngine.create_default(device=0)
e.index_documents([Document(k, "alpha bravo %d" % k) for k in range(40)])
e.set_column("year", np.arange(40, dtype=np.int64) // 4 + 1980, facetable=True)
r = e.search_queries([Query("alpha", 10), Query("alpha", 10, collapse_by="year")])
assert r[0].error is None and len(r[0].records) == 10, r[0]
assert r[1].records == [] and r[1].error and "INFX_PHASED" in r[1].error and r[1].group_values is None, r[1]
'''
    env = dict(os.environ); env["INFX_PHASED"] = "1"
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", script], check=True, env=env, timeout=300)


# ---- deletions, a restore and a replaced column ------------------------------------------------------------------------------------------------------
def test_deletions_a_restore_and_a_replaced_column_change_the_answer_as_the_model_says():
    e, cols = small_engine(300)
    vals = cols["ten"][0]
    q = Query("alpha", 20, 500, True, coverage_setup=NO_TRUNCATE, collapse_by="ten", collapse_keep=2)

    def check(vals, ctx):
        l_res = e.search_queries([q0_of(q)])[0]
        r = e.search_queries([q])[0]
        assert_collapsed(r, rows_of(l_res), flags_of(l_res), vals, q, ctx)
        return r, rows_of(l_res)
    first, L = check(vals, "first")
    gone = [k for k, _, _ in L[:3]] + [L[7][0]]
    assert e.delete_document_ids(gone) == len(gone)
    second, L2 = check(vals, "deleted")
    assert not set(gone) & {k for k, _, _ in L2} and rows_of(second) != rows_of(first)
    e.restore_documents()
    third, L3 = check(vals, "restored")
    assert L3 == L
    same_answer(third, first, "restored")
    other = ((np.arange(300) // 3) % 4).astype(np.int64)
    e.set_column("ten", other, facetable=True)                                       # the collapse column replaced
    fourth, _ = check(other, "replaced")
    assert fourth.total_groups == 4 and len(fourth.records) == 8
