"""The C ABI and the Python surface of Query.collapse_by (the best N ranked rows of every group) without a GPU: Query's two fields and their defaults,
Result's four plain attributes behind the pinned dataclass fields, the four engine symbols with the documented signatures, a null session refused,
infx_query_options unchanged, and field names — empty and seventeen characters long included — refused per query, not per call."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np

import infidex_amd
from infidex_amd import SearchEngine, Query, Result, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "infx_engine_set_query_collapse": "infx_session* s, uint32_t nq, const char* const* fields, const int32_t* keeps, int32_t* out_status",
    "infx_engine_last_collapse": "infx_session* s, uint32_t nq, uint32_t* total_groups, uint32_t* total_ranked",
    "infx_engine_collapse_rows": "infx_session* s, uint32_t qi, int32_t* col, uint32_t* codes, uint32_t* sizes, int32_t cap",
    "infx_engine_last_collapse_stats": "infx_session* s, uint32_t* queries, uint32_t* launches",
}
DEVICE_SIGNATURES = {
    "infx_stream_set_query_collapse": "infx_stream* s, uint32_t nq, const infx_collapse_req* reqs",
    "infx_last_collapse": "infx_stream* s, uint32_t nq, uint32_t* total_groups, uint32_t* total_ranked",
    "infx_collapse_rows": "infx_stream* s, uint32_t qi, uint32_t* codes, uint32_t* sizes, int32_t cap",
    "infx_last_collapse_stats": "infx_stream* s, uint32_t* queries, uint32_t* launches",
}
EINVAL, EUNSUPPORTED, EHIP = 1, 5, 3


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    a = E._u16("alpha beta gamma"); offs = np.asarray([0, len(a)], np.uint64)
    e.index_flat(None, a, offs)
    e.set_column("shade", ["red"], facetable=True)
    e.set_column("seventeen_letters", ["x"], facetable=False)      # (a name of seventeen characters that exists)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


def test_query_fields_and_defaults():
    names = [f.name for f in dataclasses.fields(Query)]
    assert names[-2:] == ["collapse_by", "collapse_keep"] and names[-3] == "pre_filter_facets"
    q = Query("x")
    assert q.collapse_by is None and q.collapse_keep == 1
    assert Query("x", collapse_by="shop", collapse_keep=3).collapse_keep == 3
    for owner in (SearchEngine, E.Session):
        assert hasattr(owner, "last_collapse_stats")
    assert [k for k in inspect.signature(SearchEngine.last_collapse_stats).parameters] == ["self", "session"]
    assert {"Query", "Result"} <= set(infidex_amd.__all__)


def test_result_attributes_are_plain_and_the_dataclass_fields_stay():
    assert dataclasses.fields(Result)[-1].name == "error"
    names = [f.name for f in dataclasses.fields(Result)]
    r = Result()
    for attr in ("group_values", "group_sizes", "total_groups", "total_ranked"):
        assert attr not in names and getattr(Result, attr) is None and getattr(r, attr) is None
        assert attr not in repr(r)
    a, b = Result(), Result()
    a.group_values = ["x"]; a.group_sizes = [1]; a.total_groups = 1; a.total_ranked = 1
    assert a == b                                                       # left out of ==, as pre_filter_facets is
    assert b.group_values is None


def test_symbols_are_exported_and_declared_int32_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for hdr, sigs in (("include/infidex_engine.h", SIGNATURES), ("include/infidex_hip.h", DEVICE_SIGNATURES)):
        h = header(hdr)
        for name, params in sigs.items():
            assert getattr(L, name) is not None, name
            m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, h)
            assert m, name
            got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
            assert got == params, (name, got)
        assert re.search(r"#define\s+INFX_COLLAPSE_MAX_KEEP\s+16\b", h)
    m = re.search(r"typedef struct infx_collapse_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "int32_t col; int32_t keep;"


def test_query_options_keep_their_layout():
    m = re.search(r"typedef struct infx_query_options \{([^}]*)\}", header("include/infidex_engine.h"))
    fields = [" ".join(x.split()) for x in m.group(1).split(";") if x.strip()]
    assert fields == ["int32_t max_results", "int32_t enable_coverage, enable_facets, enable_boost", "const char* filter", "uint32_t nboosts",
                      "const char* const* boost_filters", "const int32_t* boost_strengths", "const char* sort_by", "int32_t sort_ascending"]
    assert [f[0] for f in E._QueryOptions._fields_] == ["max_results", "enable_coverage", "enable_facets", "enable_boost", "filter", "nboosts", "boost_filters",
                                                        "boost_strengths", "sort_by", "sort_ascending"]
    assert not any("collapse" in f for f in fields)
    assert C.sizeof(E._QueryOptions) == 64


def test_a_null_session_is_refused():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)(); col = C.c_int32(0)
    names = (C.c_char_p * 1)(b"shade"); keeps = (C.c_int32 * 1)(1)
    assert L.infx_engine_set_query_collapse(None, 1, names, keeps, None) == EINVAL
    assert L.infx_engine_set_query_collapse(None, 0, None, None, None) == EINVAL
    assert L.infx_engine_last_collapse(None, 1, buf, buf) == EINVAL
    assert L.infx_engine_collapse_rows(None, 0, C.byref(col), buf, buf, 4) == -1
    assert L.infx_engine_last_collapse_stats(None, buf, buf) == EINVAL
    assert L.infx_stream_set_query_collapse(None, 0, None) == EINVAL
    assert L.infx_last_collapse(None, 0, None, None) == EINVAL
    assert L.infx_collapse_rows(None, 0, None, None, 0) == -1
    assert L.infx_last_collapse_stats(None, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_set_query_collapse(sh, 1, names, None, None) == EINVAL          # fields without keeps
    assert L.infx_engine_collapse_rows(sh, 0, C.byref(col), buf, buf, 4) == -1           # nothing searched yet on this session
    assert L.infx_engine_last_collapse(sh, 1, buf, buf) == EINVAL
    assert e.last_collapse_stats() == (0, 0)


def test_field_names_and_keeps_reach_the_status_of_their_query_not_the_calls():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    fields = [None, b"", b"seventeen_letterz", b"nosuch", b"shade", b"shade", b"shade", b"shade", b"seventeen_letters"]
    keeps = [1, 1, 1, 1, 0, 17, -1, 1, 16]
    assert len(b"seventeen_letterz") == 17
    names = (C.c_char_p * len(fields))(*fields); ks = (C.c_int32 * len(fields))(*keeps)
    st = np.full(len(fields), -7, np.int32)
    assert L.infx_engine_set_query_collapse(sh, len(fields), names, ks, st.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    # (a known column with a good keep gets as far as "no GPU" on this host-only engine: the request itself was in order)
    assert st.tolist() == [0, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, EHIP, EHIP]
    buf = C.create_string_buffer(512)
    assert L.infx_engine_query_error(sh, 2, buf, 512) >= 0 and b"seventeen_letterz" in buf.value
    assert L.infx_engine_query_error(sh, 4, buf, 512) >= 0 and b"collapse_keep" in buf.value
    assert L.infx_engine_set_query_collapse(sh, 0, None, None, None) == 0                # nq = 0 clears
    assert L.infx_engine_set_query_collapse(sh, 3, None, None, None) == 0                # fields == NULL: none
