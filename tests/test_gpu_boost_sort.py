"""Query.Boosts and Query.SortBy on the GPU (k_postproc after k_postfilter): SearchEngine.ApplyPostProcessing's boost and sort-by steps
(Scoring/ResultProcessor.cs:75-141, 180-201) against a test-side restatement (tests/bcl_sort.py: fp32 boost add + the BCL's unstable introsort,
itself held to the host build of the device sort in tests/test_bclsort_model.py).

The base rows of every case are the product's plain filtered rows of the same batch, which carry the oracle's keys and tiebreakers (oracle_lib
search_filtered; checked at top-20 with coverage, where the parity suites hold the order exact); the restatement applied to them gives the expected
keys, tiebreakers and score BITS."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, Query, Boost, BoostStrength
from infidex_amd.engine import InfidexError
from tests import oracle_lib as O
from tests import bcl_sort as B
from tools.synth import Synth

pytestmark = pytest.mark.gpu
GENRES = ["Action", "Comedy", "Drama", "Horror", "Sci-Fi", "Romance", "Thriller", "Western", "Fantasy", "Mystery", "Crime", "Animation", "drama", "DRAMA"]


def columns(n, seed=5):
    rng = np.random.default_rng(seed)
    year = rng.integers(1950, 2025, n).astype(np.int64)
    rating = np.round(rng.uniform(1.0, 10.0, n), 1)
    pick = rng.integers(0, 20, n)
    rating[pick == 0] = np.nan                                   # NaN sorts lowest, -0.0 == +0.0 (double.CompareTo)
    rating[pick == 1] = -0.0
    rating[pick == 2] = 0.0
    genre = [GENRES[i] for i in rng.integers(0, len(GENRES), n)]  # "Drama" / "drama" / "DRAMA": OrdinalIgnoreCase-equal, ordered by ordinal
    return year, rating, genre


class Fixture:
    def __init__(self, e, o, cols):
        self.e, self.o, self.cols = e, o, cols
        self._hit = {}

    def fields(self, doc):
        year, rating, genre = self.cols
        return {"year": int(year[doc]), "rating": float(rating[doc]), "genre": genre[doc]}

    def holds(self, expr, doc):
        k = (expr, doc)
        if k not in self._hit:
            self._hit[k] = O.filter_eval(expr, self.fields(doc))
        return self._hit[k]

    def sort_value(self, field, doc):
        year, rating, genre = self.cols
        if field == "year":
            return int(year[doc])
        if field == "rating":
            return B.double_key(float(rating[doc]))
        if field == "genre":
            return B.string_key(genre[doc])
        return None                                              # no such field: every row null

    def expected(self, base, enable_boost, boosts, sort_by, ascending):
        """SearchEngine.ApplyPostProcessing after the filter, on rows [(key, score, tie)] (the key is the document: the corpus has no explicit keys)."""
        rows = list(base)
        live = [b for b in (boosts or []) if b.filter is not None]
        if enable_boost and boosts and live:
            rows = B.apply_boosts(rows, [[int(b.strength) for b in live if self.holds(b.filter, k)] for k, _, _ in rows])
        if sort_by is not None:
            rows = B.apply_sort(rows, [self.sort_value(sort_by, k) for k, _, _ in rows], ascending)
        return rows


def rows_of(r):
    return [(x.document_id, x.score, x.tiebreaker) for x in r.records]


def assert_rows(got, want, ctx):
    assert [k for k, _, _ in got] == [k for k, _, _ in want], ctx
    assert [t for _, _, t in got] == [t for _, _, t in want], ctx
    gb = np.asarray([s for _, s, _ in got], np.float32).view(np.uint32)
    wb = np.asarray([s for _, s, _ in want], np.float32).view(np.uint32)
    assert np.array_equal(gb, wb), (ctx, gb, wb)


def run_case(F, texts, k, flt=None, enable_boost=False, boosts=None, sort_by=None, ascending=False, coverage=True, facets=True):
    """Runs the batch plain and with the boosts / sort; checks the plain rows against the oracle and the post-processed rows against the
    restatement.  Returns (plain, post) results."""
    e, o = F.e, F.o
    plain = e.search_filtered(texts, k, enable_coverage=coverage, filter=flt, enable_facets=facets)
    post = e.search_filtered(texts, k, enable_coverage=coverage, filter=flt, enable_facets=facets, enable_boost=enable_boost, boosts=boosts,
                             sort_by=sort_by, sort_ascending=ascending)
    for q, p, r in zip(texts, plain, post):
        if coverage and k <= 20:          # beyond, the parity rules allow order swaps between near-equal rows (tests/parity_classify.py): the base is the product's
            w = o.search_filtered(q, k, enable_coverage=coverage, filter=flt, enable_facets=facets)
            assert [x.document_id for x in p.records] == w["keys"], (q, flt)
            assert [x.tiebreaker for x in p.records] == w["ties"].tolist(), (q, flt)
        assert_rows(rows_of(r), F.expected(rows_of(p), enable_boost, boosts, sort_by, ascending), (q, k, flt, boosts, sort_by, ascending))
        assert r.facets == p.facets and r.total_in_filter == p.total_in_filter       # facets count the rows, whatever their order
    return plain, post


@pytest.fixture(scope="module")
def fx():
    s = Synth(2, docs=40000)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    o = O.OracleEngine.create_default(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    cols = columns(40000)
    year, rating, genre = cols
    for x in (e, o):
        x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
    qa, qo = s.queries(60, qseed=41, fuzz=0.3)
    return Fixture(e, o, cols), Synth.texts(qa, qo)


BOOSTS3 = [Boost("year >= 2000", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low), Boost("rating > 8.0", BoostStrength.Med)]


def test_boosts(fx):
    F, texts = fx
    plain, post = run_case(F, texts, 20, enable_boost=True, boosts=BOOSTS3)
    both = sum(1 for r in plain for x in r.records if F.holds("year >= 2000", x.document_id) and F.holds("genre = 'Drama'", x.document_id))
    assert both > 0                                              # overlapping boosts: rows that match two of them
    assert any(rows_of(a) != rows_of(b) for a, b in zip(plain, post))
    assert Query("x", enable_boost=True, boosts=BOOSTS3).max_boost == 6


def test_boost_matching_nothing_still_resorts(fx):
    F, texts = fx
    run_case(F, texts, 20, enable_boost=True, boosts=[Boost("year > 3000", BoostStrength.High)])


def test_null_filter_boost_and_disabled_boosts_change_nothing(fx):
    F, texts = fx
    for eb, bs in ((True, [Boost(None, BoostStrength.High)]), (False, BOOSTS3)):
        plain, post = run_case(F, texts, 20, enable_boost=eb, boosts=bs)
        for a, b in zip(plain, post):
            assert_rows(rows_of(b), rows_of(a), (eb, bs))


def test_boosts_with_filter(fx):
    F, texts = fx
    run_case(F, texts, 20, flt="year >= 1980 AND genre != 'Horror'", enable_boost=True, boosts=BOOSTS3)


@pytest.mark.parametrize("field", ["year", "rating", "genre", "nosuchfield", "Year"])
@pytest.mark.parametrize("ascending", [True, False])
def test_sort_by(fx, field, ascending):
    F, texts = fx
    plain, post = run_case(F, texts, 20, sort_by=field, ascending=ascending)
    if field in ("nosuchfield", "Year"):                         # field names are case sensitive: all null, the rows are only permuted
        for a, b in zip(plain, post):
            assert sorted(rows_of(a)) == sorted(rows_of(b))


@pytest.mark.parametrize("k", [10, 16, 17, 20, 64])
@pytest.mark.parametrize("coverage", [True, False])
def test_boosts_and_sort(fx, k, coverage):
    F, texts = fx
    run_case(F, texts[:30], k, enable_boost=True, boosts=BOOSTS3, sort_by="rating", ascending=k % 2 == 0, coverage=coverage)


def test_equal_scores_take_the_bcl_order():
    """Duplicated texts: >= 17 rows with one score, where the unstable introsort moves equal rows (the boost re-sort and every sort-by)."""
    docs = [(k, "golden apple orchard harvest") for k in range(40)] + [(k, "apple %s pie number %d" % (["red", "green", "baked"][k % 3], k)) for k in range(40, 120)]
    e = SearchEngine.create_default(device=0); e.index_documents([Document(k, t) for k, t in docs])
    o = O.OracleEngine.create_default(); o.index(docs)
    n = len(docs)
    rng = np.random.default_rng(3)
    year = rng.integers(1990, 1994, n).astype(np.int64); rating = rng.choice([1.5, 2.5, np.nan, -0.0, 0.0], n); genre = [["Drama", "drama", "Comedy"][i % 3] for i in range(n)]
    for x in (e, o):
        x.set_column("year", year, facetable=True); x.set_column("rating", rating); x.set_column("genre", genre, facetable=True)
    F = Fixture(e, o, (year, rating, genre))
    texts = ["golden apple orchard", "apple orchard harvest"]
    plain = e.search_filtered(texts, 64)
    for r in plain:
        sc = [x.score for x in r.records]
        assert max(sc.count(v) for v in set(sc)) >= 17, sc
    for k in (20, 64):
        run_case(F, texts, k, enable_boost=True, boosts=[Boost("year > 3000", BoostStrength.Low)])
        plain, post = run_case(F, texts, k, enable_boost=True, boosts=[Boost("genre = 'comedy'", BoostStrength.Low), Boost("year = 1991", BoostStrength.High)])
        for field in ("year", "rating", "genre", "nosuchfield"):
            for asc in (True, False):
                run_case(F, texts, k, sort_by=field, ascending=asc)
        run_case(F, texts, k, enable_boost=True, boosts=[Boost("year = 1992", BoostStrength.Med)], sort_by="genre", ascending=True)
    moved = e.search_filtered(texts, 20, enable_boost=True, boosts=[Boost("year > 3000", BoostStrength.Low)])
    assert any(rows_of(a) != rows_of(b) for a, b in zip(e.search_filtered(texts, 20), moved))      # equal rows really move


def test_sharded_boosts_and_sort_equal_unsharded(fx):
    from infidex_amd.engine import pack_texts
    from infidex_amd.sharded import create_sharded_engine, ShardSession, simulate_shards_dev, simulate_set_filter, simulate_set_boosts, simulate_set_sort
    F, texts = fx
    s = Synth(2, docs=40000)
    arena, offs = s.docs()
    year, rating, genre = F.cols
    W = 3
    engs = [create_sharded_engine(r, W, 0) for r in range(W)]
    for x in engs:
        x.index_flat(None, arena, offs, s.field_weights)
        x.set_column("year", year, facetable=True); x.set_column("rating", rating, facetable=False); x.set_column("genre", genre, facetable=True)
    sess = [ShardSession(x) for x in engs]
    a, off = pack_texts(texts)
    for flt, sort_by, asc in ((None, "genre", False), ("year >= 1970", "rating", True)):
        simulate_set_filter(sess, flt, True); simulate_set_boosts(sess, BOOSTS3, True); simulate_set_sort(sess, sort_by, asc)
        res = simulate_shards_dev(sess, a, off, 20)
        for r in res[1:]:
            for x, y in zip(r, res[0]):
                assert np.array_equal(x, y)
        keys, scores, ties, counts, flags = res[0]
        want = F.e.search_filtered(texts, 20, filter=flt, enable_facets=True, enable_boost=True, boosts=BOOSTS3, sort_by=sort_by, sort_ascending=asc)
        for i, w in enumerate(want):
            c = int(counts[i])
            assert_rows(list(zip(keys[i, :c].tolist(), scores[i, :c].tolist(), ties[i, :c].tolist())), rows_of(w), (texts[i], flt, sort_by))
            assert (sess[0].facets(i) or {}) == (w.facets or {})
    simulate_set_filter(sess, None, False); simulate_set_boosts(sess, None, False); simulate_set_sort(sess, None)


def test_errors(fx):
    F, texts = fx
    e = F.e
    cases = [(dict(enable_boost=True, boosts=[Boost("year >= ", BoostStrength.Low)]), 1),
             (dict(enable_boost=True, boosts=[Boost("genre MATCHES '^D'", BoostStrength.Low)]), 5),
             (dict(enable_boost=True, boosts=[Boost("year > %d" % y, BoostStrength.Low) for y in range(9)]), 4)]
    for kw, code in cases:
        with pytest.raises(InfidexError) as ei:
            e.search_filtered(texts[:2], 20, **kw)
        assert ei.value.code == code, (kw, ei.value)
    for kw in (dict(enable_boost=True, boosts=BOOSTS3), dict(sort_by="year")):
        with pytest.raises(InfidexError) as ei:
            e.search_filtered(texts[:2], 65, **kw)
        assert ei.value.code == 5
    ok = e.search_filtered(texts[:2], 20, enable_boost=True, boosts=[Boost("year > %d" % y, BoostStrength.Low) for y in range(8)] + [Boost(None, 3)])
    assert len(ok) == 2                                          # eight boosts with a filter (and a null one) are accepted
    assert len(e.search_batch(texts[:2], 65)) == 2               # nothing stays installed after an error
