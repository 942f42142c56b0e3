"""The C ABI and the Python surface of top_groups (a field's groups ranked by size, count, min, max, sum or mean, by page) without a GPU: the symbols are
exported with the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (no CPU fallback) with the refusals that need no
device — limits, offsets, group_by, by, the field — already in out_status, seventeen requests are INFX_ECAPACITY, and the three public names default to "every
live document, by size, largest first, first page of 20".  (A call that fails as a whole leaves no answers, so the refusals' messages are read on the GPU:
tests/test_gpu_top_groups.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, TopGroups, GroupRow, TopGroupsRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "infx_upload_group_rank": ("include/infidex_hip.h", "infx_index* ix, uint32_t col, uint32_t num_values, const uint32_t* rank"),
    "infx_top_groups": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_top_req* reqs, uint32_t* codes_out, infx_stats_slot* slots_out, uint32_t* counts_out, "
                        "uint32_t* group_totals_out, uint32_t* totals_out"),
    "infx_last_top_groups_info": ("include/infidex_hip.h", "infx_stream* s, uint32_t* requests, uint32_t* accumulate_passes, uint32_t* select_passes, uint32_t* launches, "
                                  "uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global"),
    "infx_engine_top_groups": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_top_request* reqs, int32_t* out_status"),
    "infx_engine_top_groups_rows": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, uint32_t* sizes, infx_stats_figures* figures, int32_t cap"),
    "infx_engine_top_groups_totals": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total_groups, uint32_t* total"),
    "infx_engine_top_groups_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_top_groups_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* accumulate_passes, uint32_t* select_passes, uint32_t* launches"),
    "infx_engine_last_top_groups_placement": ("include/infidex_engine.h", "infx_session* s, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global"),
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


def raw(group_by, by="size", field=None, filter=None, ascending=0, offset=0, limit=20):
    return E._TopReq(*[None if x is None else x.encode() for x in (filter, group_by, by, field)], ascending, offset, limit)


def test_symbols_are_exported_with_the_documented_signatures_and_struct_sizes():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    m = re.search(r"typedef struct infx_top_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == ("const uint8_t* mask; int32_t col; int32_t group_col; uint32_t by; int32_t ascending; uint32_t offset; uint32_t limit; "
                                            "uint32_t digit_bits; uint32_t reserved;")
    m = re.search(r"typedef struct infx_top_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* group_by; const char* by; const char* field; int32_t ascending; uint32_t offset; uint32_t limit;"
    assert [f[0] for f in E._TopReq._fields_] == ["filter", "group_by", "by", "field", "ascending", "offset", "limit"]
    # sizes against the header's layout: four pointers and three 32-bit fields, padded to the pointers' alignment; the figures are field_stats'
    assert C.sizeof(E._TopReq) == 48 and C.sizeof(E._StatsFigures) == 80
    for k, name in enumerate(("SIZE", "COUNT", "MIN", "MAX", "SUM", "MEAN")):
        assert re.search(r"#define\s+INFX_TOP_BY_%s\s+%d\b" % (name, k), header("include/infidex_hip.h")), name
    src = open(os.path.join(ROOT, "infidex_amd", "csrc", "top_select.h")).read()
    for k, name in enumerate(("SIZE", "COUNT", "MIN", "MAX", "SUM", "MEAN")):
        assert re.search(r"#define\s+TS_BY_%s\s+%d\b" % (name, k), src), name


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 8)()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_top_groups(None, 0, None, None, None, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad top-groups arguments"
    assert L.infx_last_top_groups_info(None, buf, buf, buf, buf, buf, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_upload_group_rank(None, 0, 0, None) == EINVAL
    assert L.infx_engine_top_groups(None, 0, None, None) == EINVAL
    assert L.infx_engine_top_groups_rows(None, 0, None, None, None, None, 0) == -1
    assert L.infx_engine_top_groups_totals(None, 0, buf, buf) == EINVAL
    assert L.infx_engine_top_groups_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_top_groups_stats(None, buf, buf, buf, buf, buf) == EINVAL
    assert L.infx_engine_last_top_groups_placement(None, buf, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_top_groups(sh, 1, None, None) == EINVAL                      # requests announced, none given
    assert L.infx_engine_top_groups_rows(sh, 0, None, None, None, None, 0) == -1      # nothing ranked yet on this session
    assert L.infx_engine_top_groups_totals(sh, 0, buf, buf) == EINVAL
    assert L.infx_engine_top_groups_error(sh, 0, None, 0) == -1
    assert e.last_top_groups_stats() == (0, 0, 0, 0, 0) and e.last_top_groups_placement() == (0, 0, 0)


def test_seventeen_requests_in_one_c_call_are_ecapacity():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    big = (E._TopReq * 17)(*[raw("shade") for _ in range(17)])
    st = np.full(17, -7, np.int32)
    assert L.infx_engine_top_groups(e._default_session(), 17, big, st.ctypes.data_as(C.POINTER(C.c_int32))) == ECAPACITY
    assert "16" in e.L.infx_engine_last_error().decode()


def test_refusals_that_need_no_device_are_einval_of_their_own_request():
    """Limit, offset, group_by, by, the field, its kind and whether it can be summed exactly are checked per request before anything needs the device: on a
    host-only engine the call as a whole is INFX_EHIP, and the requests that are wrong in themselves already carry INFX_EINVAL.  A group column may have
    any number of values: no 4096 cap."""
    L = C.CDLL(LIB_PATH)
    docs = 4100
    e = host_engine(docs)
    sh = e._default_session()
    e.set_column("wild", np.where(np.arange(docs) % 2 == 0, 1e-30, 1e30))             # about 200 binary digits
    e.set_column("edge128", np.where(np.arange(docs) % 2 == 0, 1.0, 2.0 ** 127))     # exactly 128 digits: summable
    e.set_column("edge129", np.where(np.arange(docs) % 2 == 0, 1.0, 2.0 ** 128))     # 129: not
    e.set_column("many", np.arange(docs, dtype=np.int64))                             # 4100 distinct values: a unique column
    cases = [
        (raw("shade", limit=0), EINVAL), (raw("shade", limit=1025), EINVAL), (raw("shade", offset=2 ** 31), EINVAL),
        (raw(None), EINVAL),                                                          # no group_by
        (raw("nosuch"), EINVAL),                                                      # an unknown group_by
        (raw("shade", "median", "price"), EINVAL), (raw("shade", None), EINVAL), (raw("shade", "Size"), EINVAL),      # an unknown by
        (raw("shade", "sum"), EINVAL), (raw("shade", "count"), EINVAL), (raw("shade", "mean"), EINVAL),               # a figure of a field, no field
        (raw("shade", "sum", "nosuch"), EINVAL),                                      # an unknown field
        (raw("shade", "max", "shade"), EINVAL),                                       # a string field
        (raw("shade", "size", "shade"), EINVAL),                                      # ... also where by does not need it
        (raw("shade", "sum", "wild"), EINVAL), (raw("many", "min", "edge129"), EINVAL),      # cannot be summed exactly
        (raw("shade"), 0), (raw("shade", limit=1024, offset=2 ** 31 - 1), 0), (raw("many"), 0), (raw("many", "sum", "price"), 0), (raw("many", "mean", "many"), 0),
        (raw("price", "size", "price", ascending=1), 0), (raw("shade", "max", "edge128"), 0), (raw("many", "min", "score"), 0), (raw("shade", "count", "score"), 0),
        (raw("shade", "sum", "price", "price = "), 0),                                # (a filter is not looked at before the device is needed)
    ]
    for c0 in range(0, len(cases), 16):
        part = cases[c0:c0 + 16]
        arr = (E._TopReq * len(part))(*[c[0] for c in part])
        st = np.full(len(part), -7, np.int32)
        assert L.infx_engine_top_groups(sh, len(part), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
        assert st.tolist() == [c[1] for c in part]
        buf = (C.c_uint32 * 4)()
        for which in range(len(part)):                                                # a call that failed as a whole leaves no answers for the readers
            assert L.infx_engine_top_groups_rows(sh, which, None, None, None, None, 0) == -1
            assert L.infx_engine_top_groups_totals(sh, which, buf, buf) == EINVAL
            assert L.infx_engine_top_groups_error(sh, which, None, 0) == -1


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "shade"), ("shade = 'red'", "shade", "sum", "price"), ([TopGroupsRequest("shade = 'red'", "shade"), TopGroupsRequest(None, "shade", "mean", "score", True, 3, 5)],)):
        with pytest.raises(E.InfidexError) as ei:
            e.top_groups(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_top_groups_stats() == (0, 0, 0, 0, 0)


def test_field_names_and_defaults():
    r = TopGroupsRequest()
    assert [f for f in r.__dataclass_fields__] == ["filter", "group_by", "by", "field", "ascending", "offset", "limit"]
    assert (r.filter, r.group_by, r.by, r.field, r.ascending, r.offset, r.limit) == (None, None, "size", None, False, 0, 20)
    g = GroupRow()
    assert [f for f in g.__dataclass_fields__] == ["value", "size", "count", "nan", "min", "max", "sum", "mean"]
    assert (g.value, g.size, g.count, g.nan, g.min, g.max, g.sum, g.mean) == ("", 0, None, None, None, None, None, None)
    t = TopGroups()
    assert [f for f in t.__dataclass_fields__] == ["groups", "total_groups", "total", "error"]
    assert t.groups == [] and t.total_groups == 0 and t.total == 0 and t.error is None
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.top_groups)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == \
            [("filter", None), ("group_by", None), ("by", "size"), ("field", None), ("ascending", False), ("offset", 0), ("limit", 20)]
        assert hasattr(owner, "last_top_groups_stats")
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.top_groups).parameters)[1:] == ["filter", "group_by", "by", "field", "ascending", "offset", "limit"]
    assert hasattr(ShardedSearcher, "last_top_groups_stats")
    import infidex_amd
    assert {"TopGroups", "GroupRow", "TopGroupsRequest"} <= set(infidex_amd.__all__)
