"""The C ABI and the Python surface of bucket_stats (field_stats' figures of a numeric field per range bucket of a second numeric field, over a filter)
without a GPU: the symbols are exported with the documented signatures and struct fields, their arguments are checked, a host-only engine answers INFX_EHIP
(the adding has no CPU fallback) with every refusal but the filter's already in out_status and with its message, seventeen requests are INFX_ECAPACITY, a
failed call leaves nothing for the readers, and BucketStatsRequest / BucketRow / BucketStats default to "every live document, no field, no buckets"."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, BucketStats, BucketRow, BucketStatsRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_bucket_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_bucket_stats_req* reqs, infx_stats_slot* slots_out"),
    "infx_last_bucket_stats_info": ("include/infidex_hip.h", "infx_stream* s, uint32_t* requests, uint32_t* launches, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global"),
    "infx_engine_bucket_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_bucket_stats_request* reqs, int32_t* out_status"),
    "infx_engine_bucket_stats_rows": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* sizes, infx_stats_figures* figures, int32_t cap"),
    "infx_engine_bucket_stats_whole": ("include/infidex_engine.h", "infx_session* s, uint32_t which, infx_stats_figures* out"),
    "infx_engine_bucket_stats_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_bucket_stats_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_bucket_stats_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches"),
    "infx_engine_last_bucket_stats_placement": ("include/infidex_engine.h", "infx_session* s, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global"),
}
EINVAL, EHIP, ECAPACITY = 1, 3, 4


def host_engine(docs=1):
    e = SearchEngine.create_default(device=-1, threads=1)
    texts = [E._u16("alpha beta gamma %d" % i) for i in range(docs)]
    offs = np.zeros(docs + 1, np.uint64); offs[1:] = np.cumsum([len(t) for t in texts])
    e.index_flat(None, np.concatenate(texts), offs)
    e.set_column("price", np.arange(7, 7 + docs, dtype=np.int64)); e.set_column("score", np.full(docs, 0.5)); e.set_column("shade", ["red"] * docs, facetable=True)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


KEEP = []


def raw(field, bucket_by, edges, filter=None):
    return E._BucketStatsReq(*[None if x is None else x.encode() for x in (filter, field, bucket_by)], *E._edge_arrays(edges, KEEP))


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    # the request structures, field for field; the slot and the figures are field_stats'
    m = re.search(r"typedef struct infx_bucket_stats_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "const uint8_t* mask; int32_t col; int32_t bucket_col; uint32_t nedges; uint32_t nan_ranks; uint32_t reserved; const uint32_t* thr;"
    m = re.search(r"typedef struct infx_bucket_stats_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* field; const char* bucket_by; uint32_t nedges; const int64_t* edges_i; const double* edges_d;"
    assert [f[0] for f in E._BucketStatsReq._fields_] == ["filter", "field", "bucket_by", "nedges", "edges_i", "edges_d"]
    assert C.sizeof(E._BucketStatsReq) == 48
    assert len(re.findall(r"typedef struct infx_stats_slot \{", header("include/infidex_hip.h"))) == 1
    assert len(re.findall(r"typedef struct infx_stats_figures \{", header("include/infidex_engine.h"))) == 1


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 8)(); fig = E._StatsFigures()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_bucket_stats(None, 0, None, None) == EINVAL
    assert L.infx_last_error() == b"bad bucket-stats arguments"
    assert L.infx_last_bucket_stats_info(None, buf, buf, buf, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_bucket_stats(None, 0, None, None) == EINVAL
    assert L.infx_engine_bucket_stats_rows(None, 0, None, None, 0) == -1
    assert L.infx_engine_bucket_stats_whole(None, 0, C.byref(fig)) == EINVAL
    assert L.infx_engine_bucket_stats_total(None, 0, buf) == EINVAL
    assert L.infx_engine_bucket_stats_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_bucket_stats_stats(None, buf, buf, buf) == EINVAL
    assert L.infx_engine_last_bucket_stats_placement(None, buf, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_bucket_stats(sh, 1, None, None) == EINVAL                    # requests announced, none given
    assert L.infx_engine_bucket_stats_rows(sh, 0, None, None, 0) == -1                # nothing asked yet on this session
    assert L.infx_engine_bucket_stats_whole(sh, 0, C.byref(fig)) == EINVAL
    assert L.infx_engine_bucket_stats_whole(sh, 0, None) == EINVAL
    assert L.infx_engine_bucket_stats_total(sh, 0, buf) == EINVAL
    assert L.infx_engine_bucket_stats_total(sh, 0, None) == EINVAL
    assert L.infx_engine_bucket_stats_error(sh, 0, None, 0) == -1
    assert e.last_bucket_stats_stats() == (0, 0, 0) and e.last_bucket_stats_placement() == (0, 0, 0)      # before any call


def test_refusals_are_einval_of_their_own_request():
    """The field, whether it can be summed exactly, bucket_by and the edges are checked per request, in this order, before anything needs the device: on a
    host-only engine the call as a whole is INFX_EHIP, and the requests that are wrong in themselves already carry INFX_EINVAL.  (The failed call leaves
    nothing for the readers, the messages included: their words are held by the test below and, on the GPU, by tests/test_gpu_bucket_stats.py.)"""
    L = C.CDLL(LIB_PATH)
    docs = 300
    e = host_engine(docs)
    sh = e._default_session()
    e.set_column("wild", np.where(np.arange(docs) % 2 == 0, 1e-30, 1e30))             # about 200 binary digits
    e.set_column("edge128", np.where(np.arange(docs) % 2 == 0, 1.0, 2.0 ** 127))     # exactly 128 digits: summable
    I, Dd = (0, 10, 20), (0.0, 0.5, 1.0)
    inf = float("inf")
    cases = [
        (raw(None, "price", I), EINVAL),                                              # no field
        (raw("nosuch", "price", I), EINVAL),                                          # an unknown field
        (raw("shade", "price", I), EINVAL),                                           # a string field
        (raw("wild", "price", I), EINVAL),                                            # cannot be summed exactly
        (raw("price", None, I), EINVAL),                                              # no bucket_by
        (raw("price", "nosuch", I), EINVAL),                                          # an unknown bucket_by
        (raw("price", "shade", I), EINVAL),                                           # a string bucket_by
        (raw("price", "price", (5,)), EINVAL), (raw("price", "price", tuple(range(258))), EINVAL),      # one edge, 258 edges
        (raw("price", "price", (3, 3)), EINVAL), (raw("price", "price", (4, 3)), EINVAL),               # not increasing
        (raw("price", "price", (0.5, 1.5)), EINVAL),                                  # an int column needs Python ints
        (raw("price", "score", (0.0, float("nan"))), EINVAL),                         # a NaN edge
        (raw("price", "score", (-0.0, 0.0)), EINVAL),                                 # -0.0 and 0.0 compare equal
        (raw("price", "price", I), 0), (raw("score", "price", (0, 1)), 0), (raw("price", "score", Dd), 0), (raw("score", "score", (-inf, 0.0, inf)), 0),
        (raw("edge128", "price", tuple(range(257))), 0), (raw("price", "score", (1, 2)), 0),            # 256 buckets; ints are fine as double edges
        (raw("score", "price", I, "price = "), 0),                                    # (a filter is not looked at before the device is needed)
    ]
    arr = (E._BucketStatsReq * len(cases))(*[c[0] for c in cases[:16]])
    st = np.full(16, -7, np.int32)
    assert L.infx_engine_bucket_stats(sh, 16, arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [c[1] for c in cases[:16]]
    rest = cases[16:]
    arr = (E._BucketStatsReq * len(rest))(*[c[0] for c in rest]); st = np.full(len(rest), -7, np.int32)
    assert L.infx_engine_bucket_stats(sh, len(rest), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [c[1] for c in rest]
    buf = (C.c_uint32 * 4)(); fig = E._StatsFigures()
    for which in range(len(rest)):                                                    # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_bucket_stats_rows(sh, which, None, None, 0) == -1
        assert L.infx_engine_bucket_stats_whole(sh, which, C.byref(fig)) == EINVAL
        assert L.infx_engine_bucket_stats_total(sh, which, buf) == EINVAL
        assert L.infx_engine_bucket_stats_error(sh, which, None, 0) == -1
    assert e.last_bucket_stats_stats() == (0, 0, 0)
    big = (E._BucketStatsReq * 17)()
    assert L.infx_engine_bucket_stats(sh, 17, big, None) == ECAPACITY                 # sixteen requests per call
    assert L.infx_engine_bucket_stats(sh, 16, big, None) == EHIP


def test_the_refusals_carry_field_stats_and_range_facets_messages_naming_bucket_stats():
    """The words of every refusal, from the engine's source: bucket_stats states none of its own beyond the sum's — the field's come from numeric_field_check,
    bucket_by's and the edges' from range_request_check, which takes the call's name and the field's role and is not restated."""
    src = open(os.path.join(ROOT, "infidex_amd", "csrc", "host", "engine.cpp")).read()
    body = src.split("int32_t infx_engine_bucket_stats(")[1].split("int32_t infx_engine_bucket_stats_rows(")[0]
    assert 'numeric_field_check(S->e, "bucket_stats", "sums"' in body and 'range_request_check(S->e, as_range(i), &rq[i].bcol, &rq[i].kind, &why, "bucket_stats", "bucket_by field")' in body
    assert "range_thresholds(" in body and "stats_figures(" in body and "strictly increasing" not in body and "string column" not in body
    assert src.count("static int32_t range_request_check(") == 1 and src.count("static std::vector<uint32_t> range_thresholds(") == 1
    assert 'const std::string& what = "range_facets"' in src and 'const std::string& role = "field"' in src      # range_facets' own messages are the defaults


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "price", "price", (0, 10)), ("shade = 'red'", "score", "price", (0, 5, 10)),
                 ([BucketStatsRequest("shade = 'red'", "price", "score", (0.0, 1.0)), BucketStatsRequest(None, "score", "price", (1, 2))],)):
        with pytest.raises(E.InfidexError) as ei:
            e.bucket_stats(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value) and "bucket_stats" in str(ei.value)      # with a message
    assert e.last_bucket_stats_stats() == (0, 0, 0)


def test_defaults_and_signatures():
    r = BucketStatsRequest()
    assert (r.filter, r.field, r.bucket_by, r.edges) == (None, None, None, ())
    assert BucketStatsRequest("a = 1", "price", "day", (0, 7)).bucket_by == "day"
    row = BucketRow()
    assert (row.size, row.count, row.nan, row.min, row.max, row.sum, row.mean) == (0, 0, 0, None, None, 0, None)
    b = BucketStats()
    assert (b.edges, b.buckets, b.below, b.above, b.nan, b.whole, b.total, b.error) == ((), [], row, row, row, row, 0, None)
    assert b.below is not b.above                                                     # (default rows are objects of their own)
    assert [x.name for x in dataclasses.fields(BucketStatsRequest)] == ["filter", "field", "bucket_by", "edges"]
    assert [x.name for x in dataclasses.fields(BucketRow)] == ["size", "count", "nan", "min", "max", "sum", "mean"]
    assert [x.name for x in dataclasses.fields(BucketStats)] == ["edges", "buckets", "below", "above", "nan", "whole", "total", "error"]
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.bucket_stats)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == [("filter", None), ("field", None), ("bucket_by", None), ("edges", ())]
        assert callable(owner.last_bucket_stats_stats)
    assert "session" in inspect.signature(SearchEngine.bucket_stats).parameters
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.bucket_stats).parameters)[1:] == ["filter", "field", "bucket_by", "edges"]
    assert callable(ShardedSearcher.last_bucket_stats_stats)
    # Python passes integer edges only for Python ints, as range_facets does: one function packs both
    keep = []
    n, ei, ed = E._edge_arrays((1, 2, 3), keep)
    assert n == 3 and [ei[i] for i in range(3)] == [1, 2, 3] and [ed[i] for i in range(3)] == [1.0, 2.0, 3.0]
    assert E._edge_arrays((1, 2.0), keep)[1] is None and E._edge_arrays((True, 2), keep)[1] is None and E._edge_arrays((), keep)[:2] == (0, None)
