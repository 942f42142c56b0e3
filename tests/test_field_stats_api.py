"""The C ABI and the Python surface of field_stats (counts, min / max and the exact sum and mean of a numeric field over a filter, whole or per group)
without a GPU: the symbols are exported with the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (the adding
has no CPU fallback) with every refusal but the filter's already in out_status, seventeen requests are INFX_ECAPACITY, a failed call leaves nothing for
the readers, and StatsRequest / FieldStats / GroupStats default to "every live document, no field, no group"."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, FieldStats, GroupStats, StatsRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_upload_column_values": ("include/infidex_hip.h", "infx_index* idx, uint32_t col, uint32_t num_values, const uint64_t* bits, int32_t kind, int32_t scale_exp, uint32_t nlimbs"),
    "infx_field_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_stats_req* reqs, infx_stats_slot* slots_out"),
    "infx_last_field_stats_info": ("include/infidex_hip.h", "infx_stream* s, uint32_t* requests, uint32_t* launches"),
    "infx_engine_field_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_stats_request* reqs, int32_t* out_status"),
    "infx_engine_field_stats_whole": ("include/infidex_engine.h", "infx_session* s, uint32_t which, infx_stats_figures* out"),
    "infx_engine_field_stats_groups": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, infx_stats_figures* figures, int32_t cap"),
    "infx_engine_field_stats_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_field_stats_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_field_stats_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches"),
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


def raw(field, group_by=None, filter=None):
    return E._StatsReq(*[None if x is None else x.encode() for x in (filter, field, group_by)])


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    # the request, slot and figure structures, field for field
    m = re.search(r"typedef struct infx_stats_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "const uint8_t* mask; int32_t col; int32_t group_col;"
    m = re.search(r"typedef struct infx_stats_slot \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "uint32_t finite; uint32_t nan; uint32_t pinf; uint32_t ninf; uint32_t min_rank; uint32_t max_rank; int64_t sum[INFX_STATS_MAX_LIMBS];"
    m = re.search(r"typedef struct infx_stats_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* field; const char* group_by;"
    assert [f[0] for f in E._StatsReq._fields_] == ["filter", "field", "group_by"]
    m = re.search(r"typedef struct infx_stats_figures \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == ("uint32_t count; uint32_t nan; int32_t kind; int32_t reserved; int64_t min_i; int64_t max_i; double min_d; double max_d; "
                                            "double sum_d; uint64_t sum_lo; int64_t sum_hi; double mean;")
    assert [f[0] for f in E._StatsFigures._fields_] == ["count", "nan", "kind", "reserved", "min_i", "max_i", "min_d", "max_d", "sum_d", "sum_lo", "sum_hi", "mean"]
    assert C.sizeof(E._StatsFigures) == 80
    assert re.search(r"#define\s+INFX_STATS_MAX_GROUPS\s+4096\b", header("include/infidex_hip.h")) and re.search(r"#define\s+INFX_STATS_MAX_LIMBS\s+4\b", header("include/infidex_hip.h"))


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)(); fig = E._StatsFigures()
    assert L.infx_upload_column_values(None, 0, 0, None, 1, 0, 1) == EINVAL
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_field_stats(None, 0, None, None) == EINVAL
    assert L.infx_last_error() == b"bad field-stats arguments"
    assert L.infx_last_field_stats_info(None, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_field_stats(None, 0, None, None) == EINVAL
    assert L.infx_engine_field_stats_whole(None, 0, C.byref(fig)) == EINVAL
    assert L.infx_engine_field_stats_groups(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_field_stats_total(None, 0, buf) == EINVAL
    assert L.infx_engine_field_stats_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_field_stats_stats(None, buf, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_field_stats(sh, 1, None, None) == EINVAL                     # requests announced, none given
    assert L.infx_engine_field_stats_whole(sh, 0, C.byref(fig)) == EINVAL             # nothing asked yet on this session
    assert L.infx_engine_field_stats_whole(sh, 0, None) == EINVAL
    assert L.infx_engine_field_stats_groups(sh, 0, None, None, None, 0) == -1
    assert L.infx_engine_field_stats_total(sh, 0, buf) == EINVAL
    assert L.infx_engine_field_stats_total(sh, 0, None) == EINVAL
    assert L.infx_engine_field_stats_error(sh, 0, None, 0) == -1
    assert e.last_field_stats_stats() == (0, 0, 0)                                    # before any call


def test_refusals_are_einval_of_their_own_request():
    """The field, its kind, group_by and whether the field can be summed exactly are checked per request before anything needs the device: on a host-only
    engine the call as a whole is INFX_EHIP, and the requests that are wrong in themselves already carry INFX_EINVAL."""
    L = C.CDLL(LIB_PATH)
    docs = 4100
    e = host_engine(docs)
    sh = e._default_session()
    e.set_column("wild", np.where(np.arange(docs) % 2 == 0, 1e-30, 1e30))             # 1e-30 .. 1e30: about 200 binary digits
    e.set_column("edge128", np.where(np.arange(docs) % 2 == 0, 1.0, 2.0 ** 127))     # exactly 128 digits: summable
    e.set_column("edge129", np.where(np.arange(docs) % 2 == 0, 1.0, 2.0 ** 128))     # 129: not
    e.set_column("many", np.arange(docs, dtype=np.int64))                             # 4100 distinct values: fine as a field, too many as a group
    e.set_column("g4096", np.arange(docs, dtype=np.int64) % 4096)
    cases = [
        (raw(None), EINVAL),                                                          # no field
        (raw("nosuch"), EINVAL),                                                      # an unknown field
        (raw("shade"), EINVAL),                                                       # a string field
        (raw("price", "nosuch"), EINVAL),                                             # an unknown group_by
        (raw("price", "many"), EINVAL),                                               # more than 4096 group values
        (raw("wild"), EINVAL), (raw("edge129", "shade"), EINVAL),                     # cannot be summed exactly
        (raw("price"), 0), (raw("score", "shade"), 0), (raw("g4096", "g4096"), 0), (raw("many"), 0), (raw("price", "g4096"), 0), (raw("edge128"), 0),
        (raw("score", None, "price = "), 0),                                          # (a filter is not looked at before the device is needed)
    ]
    arr = (E._StatsReq * len(cases))(*[c[0] for c in cases])
    st = np.full(len(cases), -7, np.int32)
    assert L.infx_engine_field_stats(sh, len(cases), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [c[1] for c in cases]
    buf = (C.c_uint32 * 4)(); fig = E._StatsFigures()
    for which in range(len(cases)):                                                   # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_field_stats_whole(sh, which, C.byref(fig)) == EINVAL
        assert L.infx_engine_field_stats_groups(sh, which, None, None, None, 0) == -1
        assert L.infx_engine_field_stats_total(sh, which, buf) == EINVAL
        assert L.infx_engine_field_stats_error(sh, which, None, 0) == -1
    assert e.last_field_stats_stats() == (0, 0, 0)
    big = (E._StatsReq * 17)()
    assert L.infx_engine_field_stats(sh, 17, big, None) == ECAPACITY                  # sixteen requests per call
    assert L.infx_engine_field_stats(sh, 16, big, None) == EHIP
    # a column replaced by values of another spread is judged by the new values
    e.set_column("wild", np.full(docs, 2.5))
    one = (E._StatsReq * 1)(raw("wild")); st1 = np.full(1, -7, np.int32)
    assert L.infx_engine_field_stats(sh, 1, one, st1.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP and st1.tolist() == [0]


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "price"), ("shade = 'red'", "score", "shade"), ([StatsRequest("shade = 'red'", "price", "shade"), StatsRequest(None, "score")],)):
        with pytest.raises(E.InfidexError) as ei:
            e.field_stats(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_field_stats_stats() == (0, 0, 0)


def test_defaults_and_signatures():
    r = StatsRequest()
    assert (r.filter, r.field, r.group_by) == (None, None, None)
    assert StatsRequest("a = 1", "price", "tag").group_by == "tag"
    f = FieldStats()
    assert (f.count, f.nan, f.total, f.min, f.max, f.sum, f.mean, f.groups, f.error) == (0, 0, 0, None, None, 0, None, [], None)
    g = GroupStats()
    assert (g.value, g.count, g.nan, g.min, g.max, g.sum, g.mean) == ("", 0, 0, None, None, 0, None)
    assert [x.name for x in dataclasses.fields(StatsRequest)] == ["filter", "field", "group_by"]
    assert [x.name for x in dataclasses.fields(FieldStats)] == ["count", "nan", "total", "min", "max", "sum", "mean", "groups", "error"]
    assert [x.name for x in dataclasses.fields(GroupStats)] == ["value", "count", "nan", "min", "max", "sum", "mean"]
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.field_stats)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == [("filter", None), ("field", None), ("group_by", None)]
        assert callable(owner.last_field_stats_stats)
    assert "session" in inspect.signature(SearchEngine.field_stats).parameters
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.field_stats).parameters)[1:] == ["filter", "field", "group_by"]
    assert callable(ShardedSearcher.last_field_stats_stats)
    # the composition Python does itself: the int column's sum from its two halves
    def figures(**kw):
        return E._stats_figures(np.frombuffer(E._StatsFigures(**kw), E._STATS_FIGURES)[0].tolist())
    assert E._STATS_FIGURES.itemsize == C.sizeof(E._StatsFigures) and list(E._STATS_FIGURES.names) == [f[0] for f in E._StatsFigures._fields_]
    got = figures(count=3, nan=0, kind=1, min_i=-5, max_i=9, sum_lo=2 ** 64 - 2, sum_hi=-1, mean=-2.0 / 3)
    assert got == (3, 0, -5, 9, -2, -2.0 / 3) and type(got[4]) is int and type(got[2]) is int
    assert figures(count=2, nan=0, kind=1, min_i=0, max_i=2 ** 63 - 1, sum_lo=5, sum_hi=3, mean=1.0)[4] == 3 * 2 ** 64 + 5
    got = figures(count=0, nan=2, kind=2)
    assert got == (0, 2, None, None, 0.0, None) and type(got[4]) is float
