"""CoverageSetup without a GPU: the Python dataclass and its C struct, validation on a host-only engine, the host side of the engine-wide members
(WordMatcher lookup without affix matches, PrepareQuery under MinWordSize, the LCS tolerance), and the POWER CHECK of the GPU tests — for every setup they
hold to the oracle, the oracle's own answers on the test inputs differ from its default answers, so that equality with the oracle says something."""
import ctypes as C

import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, CoverageSetup, InfidexError
from infidex_amd.engine import _CoverageSetup, _coverage_struct, _p, _u16
from tests import oracle_lib as O
from tests import oracle_setup as S

EINVAL, EUNSUPPORTED = 1, 5


def test_defaults_are_the_reference_s():      # Coverage/CoverageSetup.cs:6-103
    d = CoverageSetup()
    assert (d.min_word_size, d.levenshtein_max_word_size, d.num_typos, d.min_length_one_typo, d.min_length_two_typos) == (2, 20, 2, 3, 7)
    assert (d.coverage_min_word_hits_abs, d.coverage_min_word_hits_relative, d.coverage_q_limit_for_error_tolerance) == (1, 0, 5)
    assert d.coverage_lcs_error_tolerance_relativeq == 0.2
    assert (d.cover_whole_query, d.cover_whole_words, d.cover_fuzzy_words, d.cover_joined_words, d.cover_prefix_suffix) == (True,) * 5
    assert d.truncate is True and d.enable_lexical_prescreen is False and d.truncation_score == 254 and d.coverage_depth == 500
    assert CoverageSetup.create_default() == d


def test_create_minimal():                    # CoverageSetup.cs:153-162
    m = CoverageSetup.create_minimal()
    assert m == CoverageSetup(cover_whole_words=True, cover_fuzzy_words=False, cover_joined_words=False, cover_prefix_suffix=False, cover_whole_query=False)
    assert m.truncate and m.num_typos == 2 and m.min_word_size == 2


def test_struct_layout_matches_the_header():
    e = SearchEngine.create_default(device=-1)
    assert C.sizeof(_CoverageSetup) == e.L.infx_sizeof_coverage_setup() == 72
    offs = {n: getattr(_CoverageSetup, n).offset for n, _ in _CoverageSetup._fields_}
    assert offs["coverage_lcs_error_tolerance_relativeq"] == 32 and offs["cover_whole_query"] == 40 and offs["truncation_score"] == 68
    assert len(_CoverageSetup._fields_) == 17 and sum(1 for _, t in _CoverageSetup._fields_ if t is C.c_double) == 1
    st = _CoverageSetup(); assert e.L.infx_coverage_setup_default(C.byref(st)) == 0
    for n, _ in _CoverageSetup._fields_:
        assert getattr(st, n) == getattr(CoverageSetup(), n), n
    # every member arrives where it belongs: distinct values in, the same values out
    cs = CoverageSetup(3, 19, 1, 4, 9, 2, 1, 6, 0.35, False, True, False, True, False, False, False, 200)
    e.set_coverage_setup(cs)
    assert e.coverage_setup() == cs
    e.set_coverage_setup(None)
    assert e.coverage_setup() == CoverageSetup()


def test_host_only_engine_validates():
    e = SearchEngine(device=-1, coverage_setup=CoverageSetup(num_typos=1))
    assert e.coverage_setup().num_typos == 1
    for bad in (CoverageSetup(min_word_size=-1), CoverageSetup(num_typos=65536), CoverageSetup(levenshtein_max_word_size=1 << 20), CoverageSetup(coverage_min_word_hits_abs=-3),
                CoverageSetup(coverage_q_limit_for_error_tolerance=70000), CoverageSetup(truncation_score=256), CoverageSetup(truncation_score=-1),
                CoverageSetup(coverage_lcs_error_tolerance_relativeq=-0.1), CoverageSetup(coverage_lcs_error_tolerance_relativeq=float("nan")),
                CoverageSetup(coverage_lcs_error_tolerance_relativeq=float("inf")), CoverageSetup(min_length_two_typos=2 ** 40)):
        with pytest.raises(InfidexError) as x:
            e.set_coverage_setup(bad)
        assert x.value.code == EINVAL, bad
        assert e.coverage_setup().num_typos == 1          # a refused setup changes nothing
    e.set_coverage_setup(CoverageSetup(min_word_size=0, num_typos=65535, truncation_score=0, coverage_lcs_error_tolerance_relativeq=0.0))      # the range's ends
    with pytest.raises(InfidexError) as x:
        SearchEngine(device=-1, coverage_setup=CoverageSetup(truncation_score=300))
    assert x.value.code == EINVAL


def test_lexical_prescreen_is_refused():
    e = SearchEngine.create_default(device=-1)
    with pytest.raises(InfidexError) as x:
        e.set_coverage_setup(CoverageSetup(enable_lexical_prescreen=True))
    assert x.value.code == EUNSUPPORTED
    # per query: that query alone, with its status and its message
    sh = e._default_session()
    sts = [None, _coverage_struct(CoverageSetup(enable_lexical_prescreen=True)), _coverage_struct(CoverageSetup(truncate=False)), _coverage_struct(CoverageSetup(truncation_score=999))]
    ptrs = (C.POINTER(_CoverageSetup) * 4)(*[C.pointer(s) if s is not None else None for s in sts])
    status = np.full(4, -1, np.int32)
    assert e.L.infx_engine_set_query_coverage(sh, 4, ptrs, _p(status, C.c_int32)) == 0
    assert status.tolist() == [0, EUNSUPPORTED, 0, EINVAL]
    buf = C.create_string_buffer(256)
    assert e.L.infx_engine_query_error(sh, 1, buf, 256) > 0 and b"LexicalPrescreen" in buf.value
    assert e.L.infx_engine_query_error(sh, 0, buf, 256) == 0 and e.L.infx_engine_query_error(sh, 2, buf, 256) == 0
    assert e.L.infx_engine_query_error(sh, 3, buf, 256) > 0 and b"TruncationScore" in buf.value
    assert e.L.infx_engine_set_query_coverage(sh, 0, None, None) == 0


@pytest.fixture(scope="module")
def small():
    from tools.synth import Synth
    s = Synth(2, docs=3000)
    arena, offs = s.docs()
    o = S.oracle_engine(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    return s, arena, offs, o, Synth.texts(*s.queries(60, qseed=43, fuzz=0.3))


def test_wordmatcher_without_affix_matches(small):
    """CoverPrefixSuffix off: WordMatcherLookup.Execute makes no LookupAffix call (WordMatcherLookup.cs:51) — the ids are the union of WordMatcher.Lookup over the words."""
    s, arena, offs, o, qs = small
    e = SearchEngine(device=-1, coverage_setup=CoverageSetup(cover_prefix_suffix=False)); e.index_flat(None, arena, offs, s.field_weights)
    d = SearchEngine(device=-1); d.index_flat(None, arena, offs, s.field_weights)
    fewer = 0
    for q in qs:
        want = set()
        for w in q.split():
            if len(w) >= 2:
                r = o.wm_lookup(w, affix=False)
                if r is not None:
                    want |= set(r.tolist())
        assert e.wordmatcher(q).tolist() == sorted(want), q
        assert d.wordmatcher(q).tolist() == o.wordmatcher(q).tolist(), q
        fewer += len(want) < len(d.wordmatcher(q))
    assert fewer > 0          # the affix lists do contribute on this input


def _cov_query(e, q):
    sz = e.L.infx_sizeof_cov_query(); a = _u16(q); buf = (C.c_uint8 * sz)()
    assert e.L.infx_engine_prepare_cov_query(e.h, _p(a, C.c_uint16), len(a), buf) == 0
    raw = bytes(buf); o = 1024
    tl, nt = (int(x) for x in np.frombuffer(raw, np.int32, 2, o))
    off = np.frombuffer(raw, np.uint16, 32, o + 8)[:nt].tolist(); ln = np.frombuffer(raw, np.uint16, 32, o + 72)[:nt].tolist()
    nf = int(np.frombuffer(raw, np.int32, 2, o + 392)[1]); tol = int(np.frombuffer(raw, np.int32, 1, o + 656)[0])
    return tl, [q[a_:a_ + b_] for a_, b_ in zip(off, ln)], nf, tol


def test_prepare_query_under_the_engine_setup(small):
    """PrepareQuery tokenises with the engine-wide MinWordSize (the oracle's TermsCount under the same setup), the fusion tokens stay unfiltered, and the
    LCS tolerance follows QLimit / Relativeq (the LCS the oracle's pipeline computes for its first document under the same setup)."""
    s, arena, offs, o, qs = small
    qs = qs[:30] + ["ab cde fghi ab", "xy cdef xy"]
    for cs in (CoverageSetup(min_word_size=3), CoverageSetup(coverage_q_limit_for_error_tolerance=12, coverage_lcs_error_tolerance_relativeq=0.5),
               CoverageSetup(coverage_lcs_error_tolerance_relativeq=0.9), CoverageSetup(coverage_lcs_error_tolerance_relativeq=0.0), CoverageSetup()):
        e = SearchEngine(device=-1, coverage_setup=cs); e.index_flat(None, arena, offs, s.field_weights)
        S.set_setup(o, cs); o.set_trace(True)
        try:
            for q in qs:
                tl, toks, nf, tol = _cov_query(e, q)
                want = list(dict.fromkeys(w for w in q.split() if len(w) >= cs.min_word_size))
                assert toks == want and nf == len(q.split()) and tl == len(q), (q, toks)
                assert tol == (int(len(q) * cs.coverage_lcs_error_tolerance_relativeq) if len(q) >= cs.coverage_q_limit_for_error_tolerance else 0), q
                r = o.search(q, 10)
                if r["used_coverage"]:
                    ids, base, sc, ties, feat = o.last_trace()
                    if len(ids):
                        assert int(feat[0, 1]) == len(toks), q                      # the oracle's token count under this setup
                        texts = [arena[int(offs[i]):int(offs[i + 1])].tobytes().decode("utf-16-le") for i in ids[:1].tolist()]
                        if int(feat[0, 24]):                                         # a row whose LCS the pipeline computed: the same tolerance reproduces it
                            assert int(feat[0, 24]) == O.lcs(q, texts[0].lower(), tol), (q, texts[0], tol)
        finally:
            S.set_setup(o, CoverageSetup())


# ---- power check: the oracle's answers under each setup differ from its default answers on the inputs the GPU tests use --------------------------
def _answers(o, qs, cs, k=20):
    S.set_setup(o, cs)
    try:
        return [S.answer(S.search(o, q, k)) for q in qs]
    finally:
        S.set_setup(o, CoverageSetup())


def test_every_setup_changes_the_oracle_s_answers():
    s, arena, offs = S.synth_corpus()
    o = S.oracle_engine(); o.add_flat(None, arena, offs, s.field_weights); o.finalize()
    for name, qs, setups in (("S1", S.set_s1(s), S.SETUPS_S1), ("S2", S.set_s2(s), S.SETUPS_S2)):
        base = _answers(o, qs, CoverageSetup())
        for n, cs in setups:
            diff = sum(a != b for a, b in zip(_answers(o, qs, cs), base))
            print("power", name, n, diff, "of", len(qs))
            assert diff >= 1, (name, n)
            # a per-query setup of pipeline-level members gives the same answers as the engine-wide one; one of matcher members gives the default's
            per = [S.answer(S.search(o, q, 20, query_setup=cs)) for q in qs[:40]]
            assert per == (_answers(o, qs[:40], cs) if cs == S.pipeline_override(CoverageSetup(), cs) else base[:40]), (name, n)
        for n, cs in S.SETUPS_MIN_HITS:
            assert _answers(o, qs, cs) == base, (name, n)          # (no discriminating input here, see tests/oracle_setup.py)
    qs = S.set_s1(s)
    diff = sum(a != b for a, b in zip(_answers(o, qs, CoverageSetup(truncate=False), 100), _answers(o, qs, CoverageSetup(), 100)))
    print("power S1 truncate-off at 100 rows", diff); assert diff >= 1
    h = S.oracle_engine(); h.index(S.HAND_DOCS)
    base = _answers(h, S.HAND_QUERIES, CoverageSetup())
    for n, cs in S.SETUPS_HAND:
        diff = sum(a != b for a, b in zip(_answers(h, S.HAND_QUERIES, cs), base))
        print("power hand", n, diff, "of", len(S.HAND_QUERIES)); assert diff >= 1, n
    m = S.oracle_engine(); m.index(S.MINHITS_DOCS)
    base = _answers(m, S.MINHITS_QUERIES, CoverageSetup())
    for a in (2, 3):
        assert all(x != y for x, y in zip(_answers(m, S.MINHITS_QUERIES, CoverageSetup(coverage_min_word_hits_abs=a)), base)), a
