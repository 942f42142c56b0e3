"""The C ABI and the Python surface of field_distinct (exact distinct counts of a field, whole or per group) without a GPU: the symbols are exported with
the documented signatures, the structs have the header's layout, arguments are checked, a host-only engine answers INFX_EHIP (no CPU fallback) with the
refusals that need no device — the field, group_by — already in out_status, seventeen requests are INFX_ECAPACITY, the placement setter takes 0 .. 3, and the
three public names default to "every live document, no field, the whole only".  (A call that fails as a whole leaves no answers, so the refusals' messages
are read on the GPU: tests/test_gpu_field_distinct.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, FieldDistinct, GroupDistinct, DistinctRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "infx_field_distinct": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_distinct_req* reqs, uint32_t* distinct_out, uint32_t* totals_out, "
                            "uint32_t* group_sizes_out, uint32_t* group_distinct_out"),
    "infx_last_field_distinct_info": ("include/infidex_hip.h", "infx_stream* s, uint32_t* requests, uint32_t* launches, uint32_t* lds_passes, uint32_t* bitmap_passes, uint32_t* hash_passes"),
    "infx_engine_field_distinct": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_distinct_request* reqs, int32_t* out_status"),
    "infx_engine_field_distinct_whole": ("include/infidex_engine.h", "infx_session* s, uint32_t which, infx_distinct_figures* out"),
    "infx_engine_field_distinct_groups": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, infx_distinct_figures* figures, int32_t cap"),
    "infx_engine_field_distinct_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_field_distinct_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_field_distinct_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* lds_passes, uint32_t* bitmap_passes, "
                                              "uint32_t* hash_passes, uint32_t* launches"),
    "infx_engine_set_distinct_placement": ("include/infidex_engine.h", "infx_session* s, int32_t mode"),
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
    return E._DistinctReq(*[None if x is None else x.encode() for x in (filter, field, group_by)])


def test_symbols_are_exported_with_the_documented_signatures_and_struct_layouts():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    m = re.search(r"typedef struct infx_distinct_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "const uint8_t* mask; int32_t col; int32_t group_col; uint32_t placement; uint32_t reserved;"
    m = re.search(r"typedef struct infx_distinct_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* field; const char* group_by;"
    m = re.search(r"typedef struct infx_distinct_figures \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "uint32_t size; uint32_t distinct;"
    assert [f[0] for f in E._DistinctReq._fields_] == ["filter", "field", "group_by"] and [f[0] for f in E._DistinctFigures._fields_] == ["size", "distinct"]
    assert C.sizeof(E._DistinctReq) == 24 and C.sizeof(E._DistinctFigures) == 8 and E._DISTINCT_FIGURES.itemsize == 8
    # the structs of the siblings are what they were
    assert C.sizeof(E._StatsReq) == 24 and C.sizeof(E._StatsFigures) == 80 and C.sizeof(E._TopReq) == 48


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 8)()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_field_distinct(None, 0, None, None, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad field-distinct arguments"
    assert L.infx_last_field_distinct_info(None, buf, buf, buf, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_field_distinct(None, 0, None, None) == EINVAL
    assert L.infx_engine_field_distinct_whole(None, 0, None) == EINVAL
    assert L.infx_engine_field_distinct_groups(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_field_distinct_total(None, 0, buf) == EINVAL
    assert L.infx_engine_field_distinct_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_field_distinct_stats(None, buf, buf, buf, buf, buf, buf) == EINVAL
    assert L.infx_engine_set_distinct_placement(None, 0) == EINVAL
    e = host_engine()
    sh = e._default_session()
    fig = E._DistinctFigures()
    assert L.infx_engine_field_distinct(sh, 1, None, None) == EINVAL                      # requests announced, none given
    assert L.infx_engine_field_distinct_whole(sh, 0, C.byref(fig)) == EINVAL              # nothing counted yet on this session
    assert L.infx_engine_field_distinct_groups(sh, 0, None, None, None, 0) == -1
    assert L.infx_engine_field_distinct_total(sh, 0, buf) == EINVAL
    assert L.infx_engine_field_distinct_error(sh, 0, None, 0) == -1
    assert e.last_field_distinct_stats() == (0, 0, 0, 0, 0, 0)


def test_placement_setter_takes_zero_to_three():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    for mode, rc in ((-1, EINVAL), (0, 0), (1, 0), (2, 0), (3, 0), (4, EINVAL), (2 ** 31 - 1, EINVAL), (-2 ** 31, EINVAL)):
        assert L.infx_engine_set_distinct_placement(sh, mode) == rc, mode
    with pytest.raises(E.InfidexError) as ei:
        e.set_distinct_placement(7)
    assert ei.value.code == EINVAL
    e.set_distinct_placement(0)


def test_seventeen_requests_in_one_c_call_are_ecapacity():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    big = (E._DistinctReq * 17)(*[raw("shade") for _ in range(17)])
    st = np.full(17, -7, np.int32)
    assert L.infx_engine_field_distinct(e._default_session(), 17, big, st.ctypes.data_as(C.POINTER(C.c_int32))) == ECAPACITY
    assert "16" in e.L.infx_engine_last_error().decode()


def test_refusals_that_need_no_device_are_einval_of_their_own_request():
    """The field and group_by are checked per request before anything needs the device: on a host-only engine the call as a whole is INFX_EHIP, and the
    requests that are wrong in themselves already carry INFX_EINVAL.  The field may be any column — a string column, a unique one — and group_by is held to
    field_stats' 4096 values."""
    L = C.CDLL(LIB_PATH)
    docs = 4100
    e = host_engine(docs)
    sh = e._default_session()
    e.set_column("many", np.arange(docs, dtype=np.int64))                             # 4100 distinct values: a unique column
    e.set_column("most", np.arange(docs, dtype=np.int64) % 4096)                      # exactly 4096
    cases = [
        (raw(None), EINVAL),                                                          # no field
        (raw("nosuch"), EINVAL),                                                      # an unknown field
        (raw("price", "nosuch"), EINVAL),                                             # an unknown group_by
        (raw("price", "many"), EINVAL),                                               # a group_by of 4100 values
        (raw(None, "shade"), EINVAL), (raw("nosuch", "nosuch"), EINVAL),
        (raw("shade"), 0), (raw("many"), 0), (raw("score"), 0), (raw("price", "shade"), 0), (raw("many", "most"), 0), (raw("shade", "shade"), 0), (raw("many", "price"), EINVAL),
        (raw("most", "most"), 0),
        (raw("price", "shade", "price = "), 0),                                       # (a filter is not looked at before the device is needed)
        (raw("price", None, "shade MATCHES 'r'"), 0),
    ]
    assert len(cases) == 16
    arr = (E._DistinctReq * len(cases))(*[c[0] for c in cases])
    st = np.full(len(cases), -7, np.int32)
    assert L.infx_engine_field_distinct(sh, len(cases), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [c[1] for c in cases]
    buf = (C.c_uint32 * 4)(); fig = E._DistinctFigures()
    for which in range(len(cases)):                                                   # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_field_distinct_whole(sh, which, C.byref(fig)) == EINVAL
        assert L.infx_engine_field_distinct_groups(sh, which, None, None, None, 0) == -1
        assert L.infx_engine_field_distinct_total(sh, which, buf) == EINVAL
        assert L.infx_engine_field_distinct_error(sh, which, None, 0) == -1


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "shade"), ("shade = 'red'", "price", "shade"), ([DistinctRequest("shade = 'red'", "shade"), DistinctRequest(None, "price", "shade")],)):
        with pytest.raises(E.InfidexError) as ei:
            e.field_distinct(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_field_distinct_stats() == (0, 0, 0, 0, 0, 0)


def test_field_names_and_defaults():
    r = DistinctRequest()
    assert [f for f in r.__dataclass_fields__] == ["filter", "field", "group_by"] and (r.filter, r.field, r.group_by) == (None, None, None)
    g = GroupDistinct()
    assert [f for f in g.__dataclass_fields__] == ["value", "size", "distinct"] and (g.value, g.size, g.distinct) == ("", 0, 0)
    t = FieldDistinct()
    assert [f for f in t.__dataclass_fields__] == ["distinct", "total", "groups", "error"]
    assert t.distinct == 0 and t.total == 0 and t.groups == [] and t.error is None
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.field_distinct)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == [("filter", None), ("field", None), ("group_by", None)]
        assert hasattr(owner, "last_field_distinct_stats") and hasattr(owner, "set_distinct_placement")
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.field_distinct).parameters)[1:] == ["filter", "field", "group_by"]
    assert hasattr(ShardedSearcher, "last_field_distinct_stats")
    import infidex_amd
    assert {"FieldDistinct", "GroupDistinct", "DistinctRequest"} <= set(infidex_amd.__all__)
