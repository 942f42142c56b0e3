"""The C ABI and the Python surface of list_groups (one row per value of a field, in the order of a field, by page) without a GPU: the symbols are exported
with the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (the head pass has no CPU fallback) with the refusals that
need no device — limits outside 1 .. 1024, offsets from 2^31, a missing or unknown group_by, an unknown order_by — already in out_status, and
GroupListing / GroupListRequest default to "every live document, index order, first page of 20"."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, GroupListing, GroupListRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_list_grouped": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_group_list_req* reqs, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out, "
                          "uint32_t* gcodes_out, uint32_t* sizes_out, uint32_t* counts_out, uint32_t* group_totals_out, uint32_t* totals_out"),
    "infx_last_group_list_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* launches"),
    "infx_engine_list_groups": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_group_list_request* reqs, int32_t* out_status"),
    "infx_engine_group_list_rows": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, uint32_t* group_codes, uint32_t* sizes, int32_t cap"),
    "infx_engine_group_list_totals": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total_groups, uint32_t* total"),
    "infx_engine_group_list_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_group_list_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* launches"),
}
EINVAL, EHIP, ECAPACITY = 1, 3, 4


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    a = E._u16("alpha beta gamma"); offs = np.asarray([0, len(a)], np.uint64)
    e.index_flat(None, a, offs)
    e.set_column("shade", ["red"], facetable=True)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


def test_symbols_are_exported_and_declared_int32_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    # the request structures, field for field: the device's is infx_list_req plus group_col
    lst = re.search(r"typedef struct infx_list_req \{([^}]*)\}", header("include/infidex_hip.h"))
    grp = re.search(r"typedef struct infx_group_list_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(grp.group(1).split()) == " ".join(lst.group(1).split()) + " int32_t group_col; int32_t reserved2;"
    m = re.search(r"typedef struct infx_group_list_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* group_by; const char* order_by; int32_t ascending; uint32_t offset; uint32_t limit;"
    assert [f[0] for f in E._GroupListReq._fields_] == ["filter", "group_by", "order_by", "ascending", "offset", "limit"]


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 8)()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_list_grouped(None, 0, None, None, None, None, None, None, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad grouped-listing arguments"
    assert L.infx_last_group_list_stats(None, buf, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_list_groups(None, 0, None, None) == EINVAL
    assert L.infx_engine_group_list_rows(None, 0, None, None, None, None, None, 0) == -1
    assert L.infx_engine_group_list_totals(None, 0, buf, buf) == EINVAL
    assert L.infx_engine_group_list_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_group_list_stats(None, buf, buf, buf, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_list_groups(sh, 1, None, None) == EINVAL                     # requests announced, none given
    assert L.infx_engine_group_list_rows(sh, 0, None, None, None, None, None, 0) == -1      # nothing listed yet on this session
    assert L.infx_engine_group_list_totals(sh, 0, buf, buf) == EINVAL
    assert L.infx_engine_group_list_totals(sh, 0, None, buf) == EINVAL
    assert L.infx_engine_group_list_error(sh, 0, None, 0) == -1
    assert e.last_group_list_stats() == (0, 0, 0, 0, 0)
    big = (E._GroupListReq * 17)()
    assert L.infx_engine_list_groups(sh, 17, big, None) == ECAPACITY                  # sixteen requests per call


def test_refusals_that_need_no_device_are_einval_of_their_own_request():
    """Limits, offsets, group_by and order_by are checked per request before anything needs the device: on a host-only engine the call as a whole is
    INFX_EHIP, and the requests refused for one of them already carry INFX_EINVAL."""
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    reqs = [E._GroupListReq(None, b"shade", None, 1, 0, 0), E._GroupListReq(None, b"shade", None, 1, 0, 1025), E._GroupListReq(None, b"shade", None, 1, 0, 1),
            E._GroupListReq(None, b"shade", b"shade", 0, 0, 1024), E._GroupListReq(None, None, None, 1, 0, 20), E._GroupListReq(None, b"nosuch", None, 1, 0, 20),
            E._GroupListReq(None, b"shade", b"nosuch", 1, 0, 20), E._GroupListReq(None, b"shade", None, 1, 2 ** 31, 20), E._GroupListReq(b"shade = 'red'", b"shade", None, 1, 2 ** 31 - 1, 20)]
    arr = (E._GroupListReq * len(reqs))(*reqs)
    st = np.full(len(reqs), -7, np.int32)
    assert L.infx_engine_list_groups(sh, len(reqs), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [EINVAL, EINVAL, 0, 0, EINVAL, EINVAL, EINVAL, EINVAL, 0]
    buf = (C.c_uint32 * 4)()
    for which in range(len(reqs)):                                                    # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_group_list_rows(sh, which, None, None, None, None, None, 0) == -1
        assert L.infx_engine_group_list_totals(sh, which, buf, buf) == EINVAL
        assert L.infx_engine_group_list_error(sh, which, None, 0) == -1


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "shade"), ("shade = 'red'", "shade", "shade"), ([GroupListRequest("shade = 'red'", "shade"), GroupListRequest(None, "shade", "shade", False, 3, 5)],)):
        with pytest.raises(E.InfidexError) as ei:
            e.list_groups(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_group_list_stats() == (0, 0, 0, 0, 0)


def test_field_names_and_defaults():
    r = GroupListRequest()
    assert [f for f in r.__dataclass_fields__] == ["filter", "group_by", "order_by", "ascending", "offset", "limit"]
    assert (r.filter, r.group_by, r.order_by, r.ascending, r.offset, r.limit) == (None, None, None, True, 0, 20)
    assert GroupListRequest("a = 1", "shop", "year", False, 40, 10).limit == 10
    p = GroupListing()
    assert [f for f in p.__dataclass_fields__] == ["document_ids", "values", "group_values", "group_sizes", "total_groups", "total", "error"]
    assert p.document_ids == [] and p.values == [] and p.group_values == [] and p.group_sizes == [] and p.total_groups == 0 and p.total == 0 and p.error is None
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.list_groups)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == \
            [("filter", None), ("group_by", None), ("order_by", None), ("ascending", True), ("offset", 0), ("limit", 20)]
        assert hasattr(owner, "last_group_list_stats")
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.list_groups).parameters)[1:] == ["filter", "group_by", "order_by", "ascending", "offset", "limit"]
    assert hasattr(ShardedSearcher, "last_group_list_stats")
    import infidex_amd
    assert {"GroupListing", "GroupListRequest"} <= set(infidex_amd.__all__)
