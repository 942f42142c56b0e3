"""The C ABI and the Python surface of field_quantiles (exact medians and percentiles of a numeric field over a filter, whole and per group) without a
GPU: the symbols are exported with the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (the select has no CPU
fallback) with every refusal but the filter's already in out_status, seventeen requests are INFX_ECAPACITY, a failed call leaves nothing for the readers,
and QuantileRequest / FieldQuantiles / GroupQuantiles default to "every live document, no field, the median, no group"."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import infidex_amd
from infidex_amd import SearchEngine, FieldQuantiles, GroupQuantiles, QuantileRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_field_quantiles": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_quant_req* reqs, infx_quant_slot* slots_out, uint32_t* ranks_out"),
    "infx_last_field_quantiles_info": ("include/infidex_hip.h", "infx_stream* s, uint32_t* requests, uint32_t* hist_passes, uint32_t* launches, uint32_t* digit_bits, uint32_t* lds_rows, uint32_t* global_rows"),
    "infx_engine_field_quantiles": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_quantile_request* reqs, int32_t* out_status"),
    "infx_engine_field_quantiles_whole": ("include/infidex_engine.h", "infx_session* s, uint32_t which, infx_quantile_figures* out"),
    "infx_engine_field_quantiles_groups": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, infx_quantile_figures* figures, int32_t cap"),
    "infx_engine_field_quantiles_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_field_quantiles_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_field_quantiles_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* hist_passes, uint32_t* launches"),
    "infx_engine_last_field_quantiles_placement": ("include/infidex_engine.h", "infx_session* s, uint32_t* digit_bits, uint32_t* lds_rows, uint32_t* global_rows"),
    "infx_engine_set_quantile_digit_bits": ("include/infidex_engine.h", "infx_session* s, int32_t bits"),
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


def raw(field, q=(0.5,), group_by=None, filter=None):
    qs = np.asarray(q, np.float64); KEEP.append(qs)
    text = [None if x is None else x.encode() for x in (filter, field, group_by)]
    return E._QuantReq(text[0], text[1], text[2], qs.ctypes.data_as(C.POINTER(C.c_double)) if len(qs) else None, len(qs))


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    # the request, slot and figure structures, field for field
    m = re.search(r"typedef struct infx_quant_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == ("const uint8_t* mask; int32_t col; int32_t group_col; uint32_t nq; uint32_t digit_bits; uint32_t nan_ranks; uint32_t reserved; "
                                            "double q[INFX_QUANT_MAX];")
    m = re.search(r"typedef struct infx_quant_slot \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "uint32_t count; uint32_t nan;"
    m = re.search(r"typedef struct infx_quantile_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* field; const char* group_by; const double* q; uint32_t nq;"
    assert [f[0] for f in E._QuantReq._fields_] == ["filter", "field", "group_by", "q", "nq"]
    m = re.search(r"typedef struct infx_quantile_figures \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "uint32_t count; uint32_t nan; int32_t kind; uint32_t nq; int64_t v_i[16]; double v_d[16];"
    assert [f[0] for f in E._QuantFigures._fields_] == ["count", "nan", "kind", "nq", "v_i", "v_d"]
    assert C.sizeof(E._QuantFigures) == 16 + 2 * 16 * 8 and C.sizeof(E._QuantReq) == 40
    assert re.search(r"#define\s+INFX_QUANT_MAX\s+16\b", header("include/infidex_hip.h"))


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)(); fig = E._QuantFigures()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_field_quantiles(None, 0, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad field-quantiles arguments"
    assert L.infx_last_field_quantiles_info(None, buf, buf, buf, buf, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_field_quantiles(None, 0, None, None) == EINVAL
    assert L.infx_engine_field_quantiles_whole(None, 0, C.byref(fig)) == EINVAL
    assert L.infx_engine_field_quantiles_groups(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_field_quantiles_total(None, 0, buf) == EINVAL
    assert L.infx_engine_field_quantiles_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_field_quantiles_stats(None, buf, buf, buf, buf) == EINVAL
    assert L.infx_engine_last_field_quantiles_placement(None, buf, buf, buf) == EINVAL
    assert L.infx_engine_set_quantile_digit_bits(None, 8) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_field_quantiles(sh, 1, None, None) == EINVAL                 # requests announced, none given
    assert L.infx_engine_field_quantiles_whole(sh, 0, C.byref(fig)) == EINVAL         # nothing asked yet on this session
    assert L.infx_engine_field_quantiles_whole(sh, 0, None) == EINVAL
    assert L.infx_engine_field_quantiles_groups(sh, 0, None, None, None, 0) == -1
    assert L.infx_engine_field_quantiles_total(sh, 0, buf) == EINVAL
    assert L.infx_engine_field_quantiles_total(sh, 0, None) == EINVAL
    assert L.infx_engine_field_quantiles_error(sh, 0, None, 0) == -1
    assert e.last_field_quantiles_stats() == (0, 0, 0, 0) and e.last_field_quantiles_placement() == (0, 0, 0)      # before any call
    for bits in (3, 12, -1):
        assert L.infx_engine_set_quantile_digit_bits(sh, bits) == EINVAL
        with pytest.raises(E.InfidexError):
            e.set_quantile_digit_bits(bits)
    for bits in (4, 11, 0):                                                           # 0: the engine chooses
        assert L.infx_engine_set_quantile_digit_bits(sh, bits) == 0
        e.set_quantile_digit_bits(bits)


def test_refusals_are_einval_of_their_own_request():
    """The field, its kind, group_by and the quantiles are checked per request before anything needs the device: on a host-only engine the call as a whole
    is INFX_EHIP, and the requests that are wrong in themselves already carry INFX_EINVAL."""
    L = C.CDLL(LIB_PATH)
    docs = 4100
    e = host_engine(docs)
    sh = e._default_session()
    e.set_column("many", np.arange(docs, dtype=np.int64))                             # 4100 distinct values: fine as a field, too many as a group
    e.set_column("g4096", np.arange(docs, dtype=np.int64) % 4096)
    e.set_column("wild", np.where(np.arange(docs) % 2 == 0, 1e-30, 1e30))             # field_stats cannot sum it; its quantiles are ranks like any other's
    cases = [
        (raw(None), EINVAL),                                                          # no field
        (raw("nosuch"), EINVAL),                                                      # an unknown field
        (raw("shade"), EINVAL),                                                       # a string field
        (raw("price", (0.5,), "nosuch"), EINVAL),                                     # an unknown group_by
        (raw("price", (0.5,), "many"), EINVAL),                                       # more than 4096 group values
        (raw("price", ()), EINVAL),                                                   # q empty
        (raw("price", [i / 16 for i in range(17)]), EINVAL),                          # 17 quantiles
        (raw("price", (0.5, -0.1)), EINVAL), (raw("price", (1.5,)), EINVAL), (raw("score", (0.25, float("nan"))), EINVAL),
        (raw("score", (float("inf"),)), EINVAL), (raw("score", (-0.0, np.nextafter(1.0, 2.0))), EINVAL),
        (raw("price"), 0), (raw("score", (0.0, 1.0), "shade"), 0), (raw("g4096", (0.5,), "g4096"), 0), (raw("many", [i / 15 for i in range(16)]), 0),
        (raw("price", (-0.0, 1.0, 1.0, 0.5), "g4096"), 0), (raw("wild"), 0),
        (raw("score", (0.5,), None, "price = "), 0),                                  # (a filter is not looked at before the device is needed)
    ]
    arr = (E._QuantReq * len(cases))(*[c[0] for c in cases])
    st = np.full(len(cases), -7, np.int32)
    assert len(cases) > 16
    assert L.infx_engine_field_quantiles(sh, len(cases), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == ECAPACITY and st.tolist() == [-7] * len(cases)
    for part in (cases[:12], cases[12:]):
        arr = (E._QuantReq * len(part))(*[c[0] for c in part])
        st = np.full(len(part), -7, np.int32)
        assert L.infx_engine_field_quantiles(sh, len(part), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
        assert st.tolist() == [c[1] for c in part]
        buf = (C.c_uint32 * 4)(); fig = E._QuantFigures()
        for which in range(len(part)):                                                # a call that failed as a whole leaves no answers for the readers
            assert L.infx_engine_field_quantiles_whole(sh, which, C.byref(fig)) == EINVAL
            assert L.infx_engine_field_quantiles_groups(sh, which, None, None, None, 0) == -1
            assert L.infx_engine_field_quantiles_total(sh, which, buf) == EINVAL
            assert L.infx_engine_field_quantiles_error(sh, which, None, 0) == -1
    assert e.last_field_quantiles_stats() == (0, 0, 0, 0)
    big = (E._QuantReq * 17)()
    assert L.infx_engine_field_quantiles(sh, 17, big, None) == ECAPACITY              # sixteen requests per call
    assert L.infx_engine_field_quantiles(sh, 16, big, None) == EHIP


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "price"), ("shade = 'red'", "score", (0.1, 0.9), "shade"), ([QuantileRequest("shade = 'red'", "price", (0.5,), "shade"), QuantileRequest(None, "score")],)):
        with pytest.raises(E.InfidexError) as ei:
            e.field_quantiles(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_field_quantiles_stats() == (0, 0, 0, 0)


def test_defaults_and_signatures():
    r = QuantileRequest()
    assert (r.filter, r.field, r.q, r.group_by) == (None, None, (0.5,), None)
    assert QuantileRequest("a = 1", "price", (0.1,), "tag").group_by == "tag"
    f = FieldQuantiles()
    assert (f.q, f.values, f.count, f.nan, f.total, f.groups, f.error) == ((), [], 0, 0, 0, [], None)
    g = GroupQuantiles()
    assert (g.value, g.count, g.nan, g.values) == ("", 0, 0, [])
    assert [x.name for x in dataclasses.fields(QuantileRequest)] == ["filter", "field", "q", "group_by"]
    assert [x.name for x in dataclasses.fields(FieldQuantiles)] == ["q", "values", "count", "nan", "total", "groups", "error"]
    assert [x.name for x in dataclasses.fields(GroupQuantiles)] == ["value", "count", "nan", "values"]
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.field_quantiles)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == [("filter", None), ("field", None), ("q", (0.5,)), ("group_by", None)]
        assert callable(owner.last_field_quantiles_stats) and callable(owner.set_quantile_digit_bits)
    assert "session" in inspect.signature(SearchEngine.field_quantiles).parameters
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.field_quantiles).parameters)[1:] == ["filter", "field", "q", "group_by"]
    assert inspect.signature(ShardedSearcher.field_quantiles).parameters["q"].default == (0.5,)
    assert callable(ShardedSearcher.last_field_quantiles_stats)
    assert {"FieldQuantiles", "GroupQuantiles", "QuantileRequest"} <= set(infidex_amd.__all__)
    # what Python does itself: q as a tuple of floats (a number alone is one quantile; what is no number becomes a NaN, which the engine refuses), the values
    assert E._quantile_tuple((0, 1, 0.5)) == (0.0, 1.0, 0.5) and all(type(x) is float for x in E._quantile_tuple((0, 1)))
    assert E._quantile_tuple(0.25) == (0.25,) and E._quantile_tuple([]) == () and E._quantile_tuple(np.array([0.5, 1])) == (0.5, 1.0)
    bad = E._quantile_tuple(("x", None, 0.5))
    assert bad[0] != bad[0] and bad[1] != bad[1] and bad[2] == 0.5
    fig = E._QuantFigures(count=3, nan=1, kind=1, nq=2); fig.v_i[0] = -5; fig.v_i[1] = 2 ** 63 - 1
    got = E._quantile_figures(fig)
    assert got == (3, 1, [-5, 2 ** 63 - 1]) and all(type(x) is int for x in got[2])
    fig = E._QuantFigures(count=2, nan=0, kind=2, nq=3); fig.v_d[0] = -0.0; fig.v_d[1] = float("inf"); fig.v_d[2] = 2.5
    got = E._quantile_figures(fig)
    assert got[2] == [0.0, float("inf"), 2.5] and str(got[2][0]) == "-0.0" and all(type(x) is float for x in got[2])
    assert E._quantile_figures(E._QuantFigures(count=0, nan=4, kind=2, nq=3)) == (0, 4, [None, None, None])
