"""Query.highlight on the GPU: k_highlight's rows against tests/highlight_model.py, field for field, on SearchEngine.stored_text.

The expected Highlight of a returned row is the model's answer for (the query's normalised text, the stored text of the row's document, highlight_chars, the
engine's CoverageSetup): it never comes from the code under test.  The model itself is pinned to the oracle by tests/test_highlight_model.py.  On top of that
the features that a row's records determine (highlight_model.features) must equal k_stage2's own `feat` for every returned row Stage 2 scored — which keeps
the matchers restated in highlight.hip.inc in step with stage2.hip.inc.  Corpora are a few hundred short documents; keys are the documents' indices."""
import dataclasses
import random

import pytest

from infidex_amd import SearchEngine, Document, Query, CoverageSetup
from infidex_amd.engine import Session, normalize
from tests import highlight_model as M
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

VOCAB = ["alphabet", "newyork", "new", "york", "city", "garden", "gardening", "stone", "milestone", "river", "riverbank", "bank", "ab", "ax", "lantern",
         "northern", "light", "lighthouse", "house", "at", "harbour", "harbor", "zebra", "quartz"]
FILLER = ["f%03d" % i for i in range(200)]
LONG_WORDS = ["qw%02d" % i for i in range(33)]
# query -> what it is there for
QUERIES = ["alphabet", "new york", "newyork", "alph", "habet", "phab", "superalphabet", "alpx", "alhab", "alxpha", "alphabex", "alphxbex", "ab", "ay",
           "garden stone", "gardening milestone river", "lighthouse at harbour", "light house", "riverbank", "river bank city", "nothern lantrn", "zebra",
           "quartz zebra", "stone stone garden", "quokka", "wombat quokka", "xxxxxxxx", "xyzzyplughqq"]


def corpus():
    rng = random.Random(31)
    texts = []
    for _ in range(254):
        words = [rng.choice(VOCAB) for _ in range(rng.randint(1, 9))]
        texts.append(rng.choice([" ", ", ", " - "]).join(words))
    texts += ["new york city", "the city of new york, harbour", "york new garden", "a superalphabet", "new-york lighthouse", "bank of the river"]
    for n in (1, 32, 33, 191, 192, 193):                                  # documents of n Stage-2 words (the only ones with this word, with the two below)
        texts.append(" ".join(["quokka"] + FILLER[:n - 1]))
    texts.append(" ".join(["quokka"] * 70 + ["wombat"]))                  # one word seventy times: more occurrences than spans
    texts.append("quokka " + "x" * 600 + " wombat")                        # a word longer than every width
    texts.append(" ".join(LONG_WORDS))                                     # for the queries of 32 and 33 words
    texts.append(" ".join(LONG_WORDS[:20]))
    return texts


def engine_of(texts, **kw):
    e = SearchEngine.create_default(device=0, **kw)
    e.index_documents([Document(k, t) for k, t in enumerate(texts)])
    return e


def setup_of(cs):
    cs = cs or CoverageSetup()
    return M.Setup(cs.min_word_size, cs.levenshtein_max_word_size, cs.num_typos, cs.min_length_one_typo, cs.min_length_two_typos,
                   cs.cover_whole_words, cs.cover_fuzzy_words, cs.cover_joined_words, cs.cover_prefix_suffix)


class Texts:
    """stored_text by document, fetched once"""
    def __init__(self, e):
        self.e = e; self.t = {}

    def __getitem__(self, d):
        if d not in self.t:
            self.t[d] = self.e.stored_text(d)
        return self.t[d]


def as_dict(h):
    return dict(status=h.status, terms=[dataclasses.asdict(t) for t in h.terms], spans=[tuple(s) for s in h.spans], truncated=h.truncated,
                snippet=h.snippet, snippet_start=h.snippet_start, words=h.words)


def assert_highlights(q, r, texts, setup, seen=None, ctx=""):
    assert r.error is None, (ctx, q.text, r.error)
    assert r.highlights is not None and len(r.highlights) == len(r.records), (ctx, q.text)
    qtext = normalize(q.text, lower=True)
    for rec, h in zip(r.records, r.highlights):
        assert h.document_index == rec.document_id, (ctx, q.text)                 # keys are indices here
        want = M.highlight(qtext, texts[h.document_index], q.highlight_chars, setup)
        assert as_dict(h) == want, (ctx, q.text, h.document_index, texts[h.document_index][:200])
        if h.status != "ok":
            assert h.terms == [] and h.spans == [] and h.snippet == ""
        else:
            stored = M.units(texts[h.document_index])
            assert M.text_of(stored[h.snippet_start:h.snippet_start + len(M.units(h.snippet))]) == h.snippet
            assert len(M.units(h.snippet)) <= q.highlight_chars and len(h.spans) <= 64
        if seen is not None:
            seen["status:" + h.status] = seen.get("status:" + h.status, 0) + 1
            seen["truncated"] = seen.get("truncated", 0) + int(h.truncated)
            for t in h.terms:
                seen[t.kind] = seen.get(t.kind, 0) + 1
                if t.kind == "fuzzy_prefix":
                    seen["fp%+d" % (t.match_length - len(M.units(t.word)))] = 1
                if t.kind == "fuzzy":
                    seen["fuzzy%d" % t.distance] = 1


@pytest.fixture(scope="module")
def main():
    texts = corpus()
    e = engine_of(texts)
    return e, Texts(e), texts


def test_every_kind_every_document_length_and_truncation(main):
    e, texts, raw = main
    qs = [Query(t, 40, highlight=True) for t in QUERIES]
    res = e.search_queries(qs)
    assert e.last_highlight_stats() == (len(qs), 1)
    seen = {}
    for q, r in zip(qs, res):
        assert_highlights(q, r, texts, M.Setup(), seen)
    for kind in M.KINDS + ("fp+0", "fp+1", "fp-1", "fuzzy1", "fuzzy2", "status:ok", "status:too_long", "truncated"):
        assert seen.get(kind, 0) > 0, (kind, seen)
    words = {h.words for r in res for h in r.highlights if h.status == "ok"}
    assert {1, 32, 33, 191, 192} <= words, sorted(words)
    too_long = {h.document_index for r in res for h in r.highlights if h.status == "too_long"}
    assert too_long == {260 + 5}                                              # the document of 193 words
    assert res[QUERIES.index("xyzzyplughqq")].records == [] and res[QUERIES.index("xyzzyplughqq")].highlights == []
    ms, nbytes = e.last_highlight_timings()
    assert ms > 0 and nbytes == len(qs) * 40 * 2 * (10 + 8 * 3 + 5 * 64 + 160)      # rows strided by the batch's largest word count (3) and width (160)


def test_queries_of_1_2_32_and_33_words(main):
    e, texts, raw = main
    qs = [Query("qw00", 5, highlight=True), Query("qw00 qw01", 5, highlight=True), Query(" ".join(LONG_WORDS[:32]), 5, highlight=True),
          Query(" ".join(LONG_WORDS), 5, highlight=True)]
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        assert_highlights(q, r, texts, M.Setup())
    assert [len(r.highlights[0].terms) for r in res[:3]] == [1, 2, 32]
    assert res[3].records and all(h.status == "long_query" and h.document_index == rec.document_id for h, rec in zip(res[3].highlights, res[3].records))
    assert any(all(t.kind == "whole" for t in h.terms) for h in res[2].highlights)


@pytest.mark.parametrize("nq,rows", [(1, 1), (1, 63), (1, 64), (1, 65), (2, 65)])
def test_result_slots_across_lane_and_workgroup_boundaries(main, nq, rows):
    """nq x rows slots of the result table: 1, 63, 64, 65 and 130 — one lane each, 64 lanes a workgroup."""
    e, texts, raw = main
    qs = [Query(["garden stone", "quokka"][j], rows, coverage_setup=CoverageSetup(truncate=False), highlight=True) for j in range(nq)]
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        assert_highlights(q, r, texts, M.Setup(), ctx=(nq, rows))
    assert len(res[0].records) == rows                                        # a full query ...
    if nq == 2:
        assert 0 < len(res[1].records) < rows                                 # ... and one that returns fewer rows than asked


def test_a_batch_mixing_queries_with_and_without_and_different_widths(main):
    e, texts, raw = main
    qs = [Query("garden stone", 7, highlight=True, highlight_chars=16), Query("garden stone", 7), Query("river bank city", 3, highlight=True, highlight_chars=512),
          Query("xyzzyplughqq", 7, highlight=True), Query("alph", 9), Query("zebra quartz", 9, highlight=True, highlight_chars=33)]
    res = e.search_queries(qs)
    assert e.last_highlight_stats() == (4, 1)
    for q, r in zip(qs, res):
        if q.highlight:
            assert_highlights(q, r, texts, M.Setup())
        else:
            assert r.highlights is None and r.error is None and r.records
    assert e.last_highlight_timings()[1] == 4 * 9 * 2 * (10 + 8 * 3 + 5 * 64 + 512)
    # the same queries alone return the same highlights: a row's highlight does not depend on its neighbours
    for q, r in zip(qs, res):
        if q.highlight:
            alone = e.search_queries([q])[0]
            assert alone.highlights == r.highlights and alone.records == r.records
    plain = e.search_queries([dataclasses.replace(q, highlight=False) for q in qs])
    assert e.last_highlight_stats() == (0, 0) and e.last_highlight_timings() == (0.0, 0)
    assert all(p.highlights is None for p in plain)


def test_search_takes_the_option_and_a_session_beside_the_engines_own(main):
    e, texts, raw = main
    q = Query("lighthouse at harbour", 12, highlight=True, highlight_chars=40)
    mine = e.search(q)
    assert_highlights(q, mine, texts, M.Setup())
    s = Session(e)
    try:
        theirs = s.search_queries([q, Query("alph", 5, highlight=True)])
        assert s.last_highlight_stats() == (2, 1)
        assert theirs[0].highlights == mine.highlights and theirs[0].records == mine.records
        assert_highlights(Query("alph", 5, highlight=True), theirs[1], texts, M.Setup())
        e.search_queries([Query("alph", 5)])
        assert e.last_highlight_stats() == (0, 0) and s.last_highlight_stats() == (2, 1)      # each session reports its own last batch
    finally:
        s.close()


def test_rows_without_coverage_are_highlighted_too(main):
    e, texts, raw = main
    qs = [Query(t, 10, enable_coverage=False, highlight=True) for t in ("garden stone", "alpx", "new york", "zebra")]
    res = e.search_queries(qs)
    seen = {}
    for q, r in zip(qs, res):
        assert r.records and not r.used_coverage
        assert_highlights(q, r, texts, M.Setup(), seen)
    assert seen.get("whole", 0) and seen.get("fuzzy_prefix", 0)               # (the rows are Stage 1's; what matched in them is still Stage 2's answer)


def test_the_features_of_the_records_equal_stage_2s_own(main):
    """The cross-check against k_stage2: for every returned row that Stage 2 scored, the features the kernel's records determine are Stage 2's."""
    e, texts, raw = main
    col = {name: O.FEAT_NAMES.index(name) for name in M.FEATURES}
    qs = [Query(t, 40, highlight=True) for t in QUERIES if t != "xyzzyplughqq"]
    checked = 0
    e.set_introspection(True)
    try:
        runs = []
        for q in qs:                                                          # one query a batch: Stage 2's rows of the batch are that query's
            r = e.search_queries([q])[0]
            qo, docs, _, _, _, feat = e.last_stage2()
            assert not len(qo) or set(int(x) for x in qo) == {0}
            runs.append((r, docs, feat))
    finally:
        e.set_introspection(False)
    for j, (r, docs, feat) in enumerate(runs):
        by_row = {}
        for i in range(len(docs)):
            by_row.setdefault(int(docs[i]), i)
        for h in r.highlights:
            i = by_row.get(h.document_index)
            if i is None or h.status != "ok":
                continue
            got = M.features(h.terms, h.words)
            want = {name: int(feat[i][c]) for name, c in col.items()}
            assert got == want, (qs[j].text, h.document_index, h.terms)
            assert int(feat[i][O.FEAT_NAMES.index("TermsCount")]) == len(h.terms)
            checked += 1
    assert checked >= 200, checked


def test_alias_folding(main):
    """An index with alias characters (final sigma / sigma share an upper-case image) runs the ALIAS instantiation: λογος matches λογοσ as a whole word."""
    texts = ["λογος και εργον", "λογοσ", "εργον λογος λογοσ", "alphabet λογος"] + ["garden stone %d" % i for i in range(20)]
    e = engine_of(texts)
    t = Texts(e)
    qs = [Query("λογοσ", 10, highlight=True), Query("λογος εργον", 10, highlight=True), Query("garden", 5, highlight=True)]
    res = e.search_queries(qs)
    for q, r in zip(qs, res):
        assert_highlights(q, r, t, M.Setup())
    first = {h.document_index: h for h in res[0].highlights}
    assert first[0].terms[0].kind == "whole" and first[0].terms[0].offset == 0
    assert [s[0] for s in first[2].spans] == [6, 12]                          # both spellings are occurrences of the one matched word


@pytest.mark.parametrize("cs", [CoverageSetup.create_minimal(), CoverageSetup(num_typos=0), CoverageSetup(min_word_size=4)], ids=["minimal", "no-typos", "min-word-4"])
def test_the_engines_coverage_setup(cs):
    texts = corpus()[:120] + ["abc abd abe", "abc abd"]
    e = engine_of(texts, coverage_setup=cs)
    t = Texts(e)
    qs = [Query(x, 15, highlight=True) for x in ("alphabet", "alph", "alphabex", "new york", "newyork", "garden stone", "alpx", "abc abd")]
    res = e.search_queries(qs)
    seen = {}
    for q, r in zip(qs, res):
        assert_highlights(q, r, t, setup_of(cs), seen)
    assert seen.get("whole", 0) > 0
    if not cs.cover_prefix_suffix:
        assert set(k for k in seen if k in M.KINDS) <= {"none", "whole"}
    if cs.num_typos == 0:
        assert "fuzzy" not in seen and seen.get("prefix", 0) > 0
    if cs.min_word_size == 4:                                                  # documents (and a query) without a Stage-2 word
        empty = [h for h in res[-1].highlights if h.words == 0]
        assert res[-1].records and empty and all(h.terms == [] and h.spans == [] and h.snippet == "" for h in empty)
