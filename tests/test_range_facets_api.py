"""The C ABI and the Python surface of range_facets (bucket counts and min / max of a numeric field over a filter) without a GPU: the symbols are exported
with the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (the counting has no CPU fallback) with the field and
edge refusals of the single requests already in out_status, seventeen requests are INFX_ECAPACITY, a failed call leaves nothing for the readers, and
RangeRequest / RangeFacets default to "every live document, no field, no edges"."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, RangeFacets, RangeRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_range_counts": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_range_req* reqs, uint32_t* counts_out, uint32_t* min_rank_out, uint32_t* max_rank_out"),
    "infx_last_range_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t* requests, uint32_t* launches"),
    "infx_engine_range_facets": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_range_request* reqs, int32_t* out_status"),
    "infx_engine_range_counts": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* counts, int32_t cap, uint32_t* below, uint32_t* above, uint32_t* nan"),
    "infx_engine_range_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_range_minmax": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int32_t* kind, int64_t* lo_i, int64_t* hi_i, double* lo_d, double* hi_d"),
    "infx_engine_range_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_range_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches"),
}
EINVAL, EHIP, ECAPACITY = 1, 3, 4


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    a = E._u16("alpha beta gamma"); offs = np.asarray([0, len(a)], np.uint64)
    e.index_flat(None, a, offs)
    e.set_column("price", np.asarray([7], np.int64)); e.set_column("score", np.asarray([0.5])); e.set_column("shade", ["red"], facetable=True)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


def raw(field, edges_i=None, edges_d=None, nedges=None, filter=None, keep=None):
    """an infx_range_request over numpy arrays that `keep` holds alive"""
    ei = None if edges_i is None else np.asarray(edges_i, np.int64)
    ed = None if edges_d is None else np.asarray(edges_d, np.float64)
    keep += [ei, ed]
    n = nedges if nedges is not None else len(edges_i if edges_i is not None else edges_d)
    return E._RangeReq(None if filter is None else filter.encode(), None if field is None else field.encode(), n,
                       None if ei is None else ei.ctypes.data_as(C.POINTER(C.c_int64)), None if ed is None else ed.ctypes.data_as(C.POINTER(C.c_double)))


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    # the request structures, field for field
    m = re.search(r"typedef struct infx_range_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "const uint8_t* mask; int32_t col; uint32_t nedges; uint32_t nan_ranks; uint32_t reserved; const uint32_t* thr;"
    m = re.search(r"typedef struct infx_range_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* field; uint32_t nedges; const int64_t* edges_i; const double* edges_d;"
    assert [f[0] for f in E._RangeReq._fields_] == ["filter", "field", "nedges", "edges_i", "edges_d"]
    assert re.search(r"#define\s+INFX_RANGE_MAX_EDGES\s+257\b", header("include/infidex_hip.h")) and re.search(r"#define\s+INFX_RANGE_SLOTS\s+260\b", header("include/infidex_hip.h"))


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)(); k = C.c_int32(0)
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_range_counts(None, 0, None, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad range arguments"
    assert L.infx_last_range_stats(None, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_range_facets(None, 0, None, None) == EINVAL
    assert L.infx_engine_range_counts(None, 0, None, 0, None, None, None) == -1
    assert L.infx_engine_range_total(None, 0, buf) == EINVAL
    assert L.infx_engine_range_minmax(None, 0, C.byref(k), None, None, None, None) == EINVAL
    assert L.infx_engine_range_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_range_stats(None, buf, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_range_facets(sh, 1, None, None) == EINVAL                    # requests announced, none given
    assert L.infx_engine_range_counts(sh, 0, None, 0, None, None, None) == -1         # nothing asked yet on this session
    assert L.infx_engine_range_total(sh, 0, buf) == EINVAL
    assert L.infx_engine_range_total(sh, 0, None) == EINVAL
    assert L.infx_engine_range_minmax(sh, 0, C.byref(k), None, None, None, None) == EINVAL
    assert L.infx_engine_range_minmax(sh, 0, None, None, None, None, None) == EINVAL
    assert L.infx_engine_range_error(sh, 0, None, 0) == -1
    assert e.last_range_stats() == (0, 0, 0)                                          # before any call


def test_field_and_edge_refusals_are_einval_of_their_own_request():
    """The field, its kind and the edges are checked per request before anything needs the device: on a host-only engine the call as a whole is INFX_EHIP,
    and the requests that are wrong in themselves already carry INFX_EINVAL."""
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    keep = []
    nan, inf = float("nan"), float("inf")
    cases = [
        (raw("price", [5], [5.0], keep=keep), EINVAL),                                # 1 edge
        (raw("price", list(range(258)), [float(i) for i in range(258)], keep=keep), EINVAL),      # 258 edges
        (raw("price", [1, 5, 5, 9], [1.0, 5.0, 5.0, 9.0], keep=keep), EINVAL),       # not increasing
        (raw("price", [9, 5], [9.0, 5.0], keep=keep), EINVAL),
        (raw("score", None, [-0.0, 0.0], keep=keep), EINVAL),                         # -0.0 == 0.0 as values compare
        (raw("score", None, [0.0, nan], keep=keep), EINVAL),                          # a NaN edge
        (raw("score", None, [nan, 1.0], keep=keep), EINVAL),
        (raw("price", None, [1.0, 2.0], keep=keep), EINVAL),                          # double edges on an int column
        (raw("shade", [1, 2], [1.0, 2.0], keep=keep), EINVAL),                        # a string column
        (raw("nosuch", [1, 2], [1.0, 2.0], keep=keep), EINVAL),                       # an unknown field
        (raw(None, [1, 2], [1.0, 2.0], keep=keep), EINVAL),                           # no field
        (raw("score", None, None, nedges=2, keep=keep), EINVAL),                      # a double column without double edges
        (raw("price", [1, 2], [1.0, 2.0], keep=keep), 0),                             # 2 edges, 257 edges, +-inf on a double column, ints on a double column's side
        (raw("price", list(range(257)), [float(i) for i in range(257)], keep=keep), 0),
        (raw("score", None, [-inf, 0.0, inf], keep=keep), 0),
        (raw("score", [1, 2], [1.0, 2.0], filter="price = ", keep=keep), 0),          # (a filter is not looked at before the device is needed)
    ]
    arr = (E._RangeReq * len(cases))(*[c[0] for c in cases])
    st = np.full(len(cases), -7, np.int32)
    assert L.infx_engine_range_facets(sh, len(cases), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [c[1] for c in cases]
    buf = (C.c_uint32 * 4)(); k = C.c_int32(0)
    for which in range(len(cases)):                                                   # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_range_counts(sh, which, None, 0, None, None, None) == -1
        assert L.infx_engine_range_total(sh, which, buf) == EINVAL
        assert L.infx_engine_range_minmax(sh, which, C.byref(k), None, None, None, None) == EINVAL
        assert L.infx_engine_range_error(sh, which, None, 0) == -1
    assert e.last_range_stats() == (0, 0, 0)
    # the message of the missing integer edges, through Python: a single refused request on a host-only engine is still INFX_EHIP for the call
    big = (E._RangeReq * 17)()
    assert L.infx_engine_range_facets(sh, 17, big, None) == ECAPACITY                 # sixteen requests per call
    assert L.infx_engine_range_facets(sh, 16, big, None) == EHIP


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "price", (0, 10)), ("shade = 'red'", "score", (0.0, 1.0)), ([RangeRequest("shade = 'red'", "price", (0, 5, 10)), RangeRequest(None, "score", (0.5, 1.5))],)):
        with pytest.raises(E.InfidexError) as ei:
            e.range_facets(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_range_stats() == (0, 0, 0)


def test_python_passes_integer_edges_only_for_python_ints(monkeypatch):
    """edges_i is given when every edge is a Python int that is not a bool; edges_d always."""
    e = host_engine()
    seen = []
    real = e.L.infx_engine_range_facets

    class Spy:
        def __getattr__(self, name):
            if name != "infx_engine_range_facets":
                return getattr(e_L, name)

            def call(sh, n, arr, st):
                seen.extend((bool(arr[i].edges_i), [arr[i].edges_d[j] for j in range(arr[i].nedges)], arr[i].nedges) for i in range(n))
                return real(sh, n, arr, st)
            return call
    e_L = e.L
    monkeypatch.setattr(e, "L", Spy())
    with pytest.raises(E.InfidexError):
        e.range_facets([RangeRequest(None, "price", (1, 2, 3)), RangeRequest(None, "price", (1, 2.0)), RangeRequest(None, "price", (True, 2)),
                        RangeRequest(None, "price", (np.int64(1), 2)), RangeRequest(None, "score", (0.5, 1.5))])
    assert [s[0] for s in seen] == [True, False, False, False, False]
    assert seen[0][1] == [1.0, 2.0, 3.0] and seen[4][1] == [0.5, 1.5] and [s[2] for s in seen] == [3, 2, 2, 2, 2]


def test_defaults_and_signatures():
    r = RangeRequest()
    assert (r.filter, r.field, tuple(r.edges)) == (None, "", ())
    assert RangeRequest("a = 1", "price", (0, 10)).edges == (0, 10)
    f = RangeFacets()
    assert (tuple(f.edges), f.counts, f.below, f.above, f.nan, f.total, f.min, f.max, f.error) == ((), [], 0, 0, 0, 0, None, None, None)
    assert [x.name for x in __import__("dataclasses").fields(RangeFacets)] == ["edges", "counts", "below", "above", "nan", "total", "min", "max", "error"]
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.range_facets)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == [("filter", None), ("field", None), ("edges", ())]
        assert callable(owner.last_range_stats)
    assert "session" in inspect.signature(SearchEngine.range_facets).parameters
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.range_facets).parameters)[1:] == ["filter", "field", "edges"]
    assert callable(ShardedSearcher.last_range_stats)
