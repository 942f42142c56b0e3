"""Classification of a query whose final top-k DocumentId set differs between the HIP path and the oracle.

Used by tests/test_gpu_scale.py and by bench.py's reported set comparison.  A difference is a "tie-at-cut-off" only if the Stage-1
top-`depth` sets differ and every document in their symmetric difference scores within SCORE_RTOL*4 of the oracle's cut-off score
(the reference's own arithmetic is position dependent there: quirk Q9 + the BCL heap order).  Anything else is
"other" and is a parity failure.
"""
import numpy as np

SCORE_RTOL = 2e-6 * 32     # Stage-1 scores of an unreplayed query: ~1 ulp per term, <= 32 terms accumulated in fp32 (quirk Q9)


def classify(engine, oracle, queries, k, depth=500):
    """queries: texts whose final sets differ.  Returns a list of dicts {query, kind, detail}."""
    out = []
    engine.set_introspection(True)
    try:
        for q in queries:
            res = engine.search_batch([q], k, depth)[0]
            r = oracle.search(q, k, depth)
            ok, osc = oracle.last_stage1()
            gk, gsc = engine.last_stage1(0)
            od = dict(zip(ok.tolist(), osc.tolist())); gd = dict(zip(gk.tolist(), gsc.tolist()))
            got = [x.document_id for x in res.records]
            if set(got) == set(r["keys"]):
                out.append({"query": q, "kind": "identical-on-rerun", "detail": ""})
                continue
            sym = set(od) ^ set(gd)
            cut = min(osc) if len(osc) else 0.0
            if sym and all(abs(od.get(d, gd.get(d)) - cut) <= SCORE_RTOL * 4 * max(abs(cut), 1.0) for d in sym):
                exact = sum(1 for d in sym if np.float32(od.get(d, gd.get(d))) == np.float32(cut))
                out.append({"query": q, "kind": "tie-at-cut-off",
                            "detail": f"stage-1 symmetric difference {len(sym)} docs at cut {cut!r} ({exact} bit-equal to it); final diff {sorted(set(got) ^ set(r['keys']))}"})
            else:
                out.append({"query": q, "kind": "other",
                            "detail": f"stage-1 symmetric difference {len(sym)} docs, cut {cut!r}; final got {got} want {r['keys']}"})
    finally:
        engine.set_introspection(False)
    return out


FINAL_SCORE_TOL = 2.0 ** -6 + 1e-6     # the former bar (fp32 step of (float)precedence + semantic at precedence >= 2^17): an upper bound of every rule below


def bits(x):
    """The fp32 bit pattern of a score."""
    return int(np.float32(x).view(np.uint32))


def ulp(x):
    """One fp32 ulp of an oracle score: the step from |x| to the next larger float (np.spacing)."""
    return float(np.spacing(np.abs(np.float32(x))))


def blend_slack(score, share_diff):
    """How far a Stage-2 score may move when its BM25 share moves by `share_diff` (gap * |base difference|): the share itself, plus the rounding of the
    blend `coverageRatio * semantic + gap * base` (the product and the sum: one ulp of the semantic score, < 1, each) — oracle/coverage.hpp fusion_calculate."""
    return float(share_diff) + 2 * ulp(min(abs(float(score)), 0.999))


def final_blend_slack(score):
    """blend_slack for a final row whose base is not known: an unreplayed query's Stage-1 scores are within SCORE_RTOL of the oracle's, so base = score / maxT
    within 2 * SCORE_RTOL relative, and gap * base <= semantic <= min(score, 0.999)."""
    return blend_slack(score, 2 * SCORE_RTOL * min(abs(float(score)), 0.999))


def score_matches(got, want, coverage=True, slack=None, what=""):
    """The final-score rule.  A Stage-2 score (`coverage`) carries the oracle's bits, or lies within one ulp of the oracle's score plus `slack`: the only input
    that may differ is the Stage-1 base of the row (baseScore = score / maxT of an unreplayed query, quirk Q9), and it enters FusionScorer once
    (`partial && bm25 >= gap`, oracle/coverage.hpp) as the share gap * base.  Above precedence 1 the share's difference rounds away (one ulp at most); below,
    the score is the semantic score itself and carries it (measured: base 2 ulps apart -> score 2 ulps apart at 0.669 and at 1.93).  `slack` defaults to
    final_blend_slack.  A Stage-1 score (no coverage stage ran) is within SCORE_RTOL relative of the oracle's.  No allowance exceeds FINAL_SCORE_TOL (a Stage-2
    score is below 2^18, where one ulp is 2^-6).  Returns True when the bits are equal; fails otherwise unless the difference is within the allowance."""
    g, w = np.float32(got), np.float32(want)
    if bits(g) == bits(w):
        return True
    if coverage:
        tol = ulp(w) + (final_blend_slack(w) if slack is None else slack)
    else:
        tol = SCORE_RTOL * max(abs(float(w)), 1e-9)
    assert abs(float(g) - float(w)) <= min(tol, FINAL_SCORE_TOL), (what, "score", float(g), float(w), "diff", float(g) - float(w), "allowed", tol)
    return False


def assert_final_rows(got_keys, got_scores, want_keys, want_scores, coverage=True, what=""):
    """One query's final rows against the oracle's: identical DocumentId sets; every score by `score_matches`; the oracle's order, except that two rows may
    swap when their oracle scores are within the allowance of `score_matches` of each other AND at least one of them is not bit-equal.  The final order
    is the total order (score, tiebreaker, key), so rows that carry the oracle's bits can never swap.  Returns (rows not bit-equal, swapped pairs)."""
    got_keys = [int(x) for x in got_keys]; want_keys = [int(x) for x in want_keys]
    assert len(got_keys) == len(want_keys) and set(got_keys) == set(want_keys), (what, got_keys, want_keys)
    gs = dict(zip(got_keys, got_scores)); os_ = dict(zip(want_keys, want_scores))
    exact = {d: score_matches(gs[d], os_[d], coverage, what=(what, d)) for d in got_keys}
    swaps = 0
    if got_keys != want_keys:
        pos = {d: i for i, d in enumerate(got_keys)}
        for i, a in enumerate(want_keys):
            for b in want_keys[i + 1:]:
                if pos[a] < pos[b]:
                    continue
                swaps += 1                              # the oracle ranks a above b, the rows rank b above a
                sa, sb = float(np.float32(os_[a])), float(np.float32(os_[b]))
                lo = min(sa, sb)
                near = abs(sa - sb) <= min(ulp(lo) + final_blend_slack(lo) if coverage else SCORE_RTOL * max(abs(lo), 1e-9), FINAL_SCORE_TOL)
                assert near and not (exact[a] and exact[b]), (what, "order", a, b, sa, sb, float(gs[a]), float(gs[b]), got_keys, want_keys)
    return sum(1 for v in exact.values() if not v), swaps


def stage2_scored(oracle, r):
    """Whether the final rows of the oracle's last search `r` carry Stage-2 scores: the coverage stage ran and did not hand the Stage-1 rows back
    (it does when no candidate has a word hit, SearchPipeline.cs: `maxWordHits == 0 && wmIds.empty()`)."""
    if not r["used_coverage"]:
        return False
    ok, osc = oracle.last_stage1()
    s1 = dict(zip(ok.tolist(), osc.tolist()))
    return not all(d in s1 and bits(s1[d]) == bits(x) for d, x in zip(r["keys"], r["scores"]))


def assert_final_rows_match_oracle(keys, scores, counts, oracle, texts, k, depth=500, what=""):
    """Final rows of a product batch against the oracle, query by query (`assert_final_rows`).  Returns (identical order, queries with swapped rows,
    rows not bit-equal)."""
    same = flips = inexact = 0
    for i, q in enumerate(texts):
        r = oracle.search(q, k, depth)
        n = int(counts[i])
        bad, swaps = assert_final_rows(keys[i, :n], scores[i, :n], r["keys"], r["scores"], stage2_scored(oracle, r), (what, q))
        inexact += bad
        if swaps:
            flips += 1
        else:
            same += 1
    return same, flips, inexact
