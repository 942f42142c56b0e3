"""The C ABI and the Python surface of Query.highlight (match spans and a snippet for every returned row) without a GPU: Query's two keyword-only fields and
their defaults, Result.highlights behind the pinned dataclass fields, Highlight and TermMatch, the engine's and the device library's symbols with the documented
signatures, a null session refused, widths refused per query (not per call) with their messages and neighbours unaffected, the fifth place of the part in the
per-query frame (a query that collapse and highlight both refuse reports collapse's message), and stored_text.

(That highlight on a browse query is refused is known only when the batch runs, as for collapse_by: tests/test_gpu_highlight_compose.py.)"""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np

import infidex_amd
from infidex_amd import SearchEngine, Query, Result, Highlight, TermMatch, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "infx_engine_set_query_highlight": "infx_session* s, uint32_t nq, const int32_t* chars, int32_t* out_status",
    "infx_engine_highlight_rows": "infx_session* s, uint32_t qi, uint16_t* out, int64_t cap_u16",
    "infx_engine_last_highlight_stats": "infx_session* s, uint32_t* queries, uint32_t* launches",
    "infx_engine_last_highlight_timings": "infx_session* s, float* ms, uint64_t* bytes",
}
DEVICE_SIGNATURES = {
    "infx_stream_set_query_highlight": "infx_stream* s, uint32_t nq, const int32_t* chars",
    "infx_highlight_rows": "infx_stream* s, uint32_t qi, uint16_t* out, int64_t cap_u16",
    "infx_last_highlight_stats": "infx_stream* s, uint32_t* queries, uint32_t* launches",
    "infx_last_highlight_timings": "infx_stream* s, float* ms, uint64_t* bytes",
}
EINVAL, EUNSUPPORTED, EHIP = 1, 5, 3
TEXTS = ["Alpha  BETA, gamma", "Ärger im Straßen-Café", "x"]


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    arena, offs = E.pack_texts(TEXTS)
    e.index_flat(None, arena, offs)
    e.set_column("shade", ["red", "blue", "red"], facetable=True)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


def test_query_fields_and_defaults():
    by_name = {f.name: f for f in dataclasses.fields(Query)}
    assert by_name["highlight"].kw_only and by_name["highlight_chars"].kw_only
    q = Query("x")
    assert q.highlight is False and q.highlight_chars == 160
    q = Query("x", 20, highlight=True, highlight_chars=64)
    assert q.max_number_of_records_to_return == 20 and q.highlight is True and q.highlight_chars == 64
    # no positional parameter moved: the twelve positional fields in front of the new ones, and the three behind, are where they were
    pos = [p.name for p in inspect.signature(Query).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos[-4:] == ["pre_filter", "pre_filter_facets", "collapse_by", "collapse_keep"] and "highlight" not in pos
    for owner in (SearchEngine, E.Session):
        assert hasattr(owner, "last_highlight_stats") and hasattr(owner, "last_highlight_timings")
    assert hasattr(SearchEngine, "stored_text")
    assert {"Query", "Result", "Highlight", "TermMatch"} <= set(infidex_amd.__all__)


def test_result_highlights_is_a_plain_attribute_and_none_by_default():
    names = [f.name for f in dataclasses.fields(Result)]
    assert names[-1] == "error" and "highlights" not in names
    r = Result()
    assert Result.highlights is None and r.highlights is None and "highlights" not in repr(r)
    a, b = Result(), Result()
    a.highlights = [Highlight()]
    assert a == b and b.highlights is None
    assert [f.name for f in dataclasses.fields(Highlight)][:7] == ["status", "document_index", "terms", "spans", "truncated", "snippet", "snippet_start"]
    assert [f.name for f in dataclasses.fields(TermMatch)] == ["word", "kind", "offset", "length", "match_offset", "match_length", "distance", "offset2", "length2"]
    h = Highlight("too_long", 7)
    assert h.terms == [] and h.spans == [] and h.snippet == "" and h.document_index == 7
    assert E.HIGHLIGHT_KINDS == ("none", "whole", "joined_query", "joined_doc", "prefix", "suffix", "infix", "tail", "fuzzy_prefix", "fuzzy")


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for hdr, sigs in (("include/infidex_engine.h", SIGNATURES), ("include/infidex_hip.h", DEVICE_SIGNATURES)):
        h = header(hdr)
        for name, params in sigs.items():
            assert getattr(L, name) is not None, name
            m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, h)
            assert m, name
            assert re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split())) == params, name
        assert re.search(r"#define\s+INFX_HIGHLIGHT_MIN_CHARS\s+16\b", h) and re.search(r"#define\s+INFX_HIGHLIGHT_MAX_CHARS\s+512\b", h)
    for name in ("infx_engine_highlight_query", "infx_engine_document_text", "infx_highlight_layout"):
        assert getattr(L, name) is not None
    assert re.search(r"int64_t\s+infx_engine_document_text\s*\(", header("include/infidex_engine.h"))
    hl = open(os.path.join(ROOT, "infidex_amd", "csrc", "highlight.h")).read()
    for define, value in (("HL_MAX_SPANS", "64u"), ("HL_MIN_CHARS", "16"), ("HL_MAX_CHARS", "512"), ("HL_HDR", "10u"), ("HL_TERM", "8u"), ("HL_SPAN", "5u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (define, value), hl), define      # (what engine.py's row parser assumes)


def test_a_null_session_is_refused():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)(); chars = (C.c_int32 * 1)(160); rows = (C.c_uint16 * 8)(); ms = C.c_float(0)
    assert L.infx_engine_set_query_highlight(None, 1, chars, None) == EINVAL
    assert L.infx_engine_highlight_rows(None, 0, rows, C.c_int64(8)) == -1
    assert L.infx_engine_highlight_query(None, 0, None, None, None, None, None, None, None, None, None) == EINVAL
    assert L.infx_engine_last_highlight_stats(None, buf, buf) == EINVAL
    assert L.infx_engine_last_highlight_timings(None, C.byref(ms), None) == EINVAL
    assert L.infx_stream_set_query_highlight(None, 0, None) == EINVAL
    assert L.infx_highlight_rows(None, 0, None, C.c_int64(0)) == -1
    assert L.infx_last_highlight_stats(None, buf, buf) == EINVAL
    L.infx_engine_document_text.restype = C.c_int64
    assert L.infx_engine_document_text(None, C.c_int64(0), None, C.c_int64(0)) == -1
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_highlight_rows(sh, 0, rows, C.c_int64(8)) == -1            # nothing searched yet on this session
    assert e.last_highlight_stats() == (0, 0)


def test_widths_reach_the_status_of_their_query_not_the_calls():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    widths = [0, 15, 513, -1, 16, 512, 160]
    chars = (C.c_int32 * len(widths))(*widths)
    st = np.full(len(widths), -7, np.int32)
    assert L.infx_engine_set_query_highlight(sh, len(widths), chars, st.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    # (a width in range gets as far as "no GPU" on this host-only engine: the request itself was in order; query 0 did not ask and is unaffected)
    assert st.tolist() == [0, EINVAL, EINVAL, EINVAL, EHIP, EHIP, EHIP]
    buf = C.create_string_buffer(512)
    for i in (1, 2, 3):
        assert L.infx_engine_query_error(sh, i, buf, 512) >= 0 and b"highlight_chars is 16 .. 512" in buf.value
    assert L.infx_engine_query_error(sh, 0, buf, 512) >= 0 and buf.value == b""
    assert L.infx_engine_query_error(sh, 4, buf, 512) >= 0 and b"no GPU" in buf.value
    assert L.infx_engine_set_query_highlight(sh, 0, None, None) == 0                # nq = 0 clears
    assert L.infx_engine_set_query_highlight(sh, 3, None, None) == 0                # chars == NULL: none


def test_the_part_is_the_fifth_of_the_frame():
    """A query that the collapse requests and the highlight requests both refuse reports collapse's message, whichever was installed first; one that only
    highlight refuses reports highlight's."""
    L = C.CDLL(LIB_PATH)
    buf = C.create_string_buffer(512)
    for highlight_first in (False, True):
        e = host_engine()
        sh = e._default_session()
        names = (C.c_char_p * 2)(b"nosuch", None); keeps = (C.c_int32 * 2)(1, 1); chars = (C.c_int32 * 2)(15, 600)
        calls = [lambda: L.infx_engine_set_query_collapse(sh, 2, names, keeps, None), lambda: L.infx_engine_set_query_highlight(sh, 2, chars, None)]
        for call in (reversed(calls) if highlight_first else calls):
            assert call() == 0
        assert L.infx_engine_query_error(sh, 0, buf, 512) >= 0 and b"collapse_by: no field named 'nosuch'" in buf.value
        assert L.infx_engine_query_error(sh, 1, buf, 512) >= 0 and b"highlight_chars" in buf.value
    src = open(os.path.join(ROOT, "infidex_amd", "csrc", "host", "engine.cpp")).read()
    assert re.search(r"enum \{ QP_OPTIONS, QP_COVERAGE, QP_PREFILTERS, QP_COLLAPSE, QP_HIGHLIGHT, QP_PARTS \}", src)
    assert '"collapse requests", "highlight requests"}' in src


def test_a_batch_of_another_size_is_refused_and_clears_the_part():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    chars = (C.c_int32 * 2)(160, 160)
    assert L.infx_engine_set_query_highlight(sh, 2, chars, None) == 0
    try:
        e.search_batch(["alpha"], 5)
        raise AssertionError("a batch of another size ran")
    except infidex_amd.InfidexError as err:
        assert "highlight requests were installed for a batch of another size" in str(err)


def test_stored_text_is_the_normalised_lower_cased_text():
    e = host_engine()
    for i, t in enumerate(TEXTS):
        assert e.stored_text(i) == E.normalize(t, lower=True)
    assert e.stored_text(0) == "alpha beta, gamma"       # (normalisation also folds the run of spaces: offsets are the stored text's, not the input's)
    for bad in (-1, len(TEXTS)):
        try:
            e.stored_text(bad)
            raise AssertionError("an index out of range was accepted")
        except infidex_amd.InfidexError:
            pass
