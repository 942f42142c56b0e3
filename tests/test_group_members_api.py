"""The C ABI and the Python surface of list_group_members (the first N documents of every group, by page) without a GPU: the symbols are exported with the
documented signatures, the device's request is infx_group_list_req plus per_group, arguments are checked, a host-only engine answers INFX_EHIP (the walks have
no CPU fallback) with the refusals that need no device — per_group outside 1 .. 16, limit * per_group beyond 4096 and list_groups' own — already in
out_status, and GroupMembersRequest defaults to "every live document, index order, three members per group, first page of 20"."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, GroupMembersListing, GroupMembers, GroupMembersRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_list_group_members": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_group_members_req* reqs, int32_t* rows_out, uint32_t* gcodes_out, uint32_t* sizes_out, "
                                "uint32_t* member_counts_out, int64_t* member_keys_out, int32_t* member_docs_out, uint32_t* member_codes_out, "
                                "uint32_t* counts_out, uint32_t* group_totals_out, uint32_t* totals_out"),
    "infx_last_group_members_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* member_walks, uint32_t* launches"),
    "infx_engine_list_group_members": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_group_members_request* reqs, int32_t* out_status"),
    "infx_engine_group_members_rows": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* group_codes, uint32_t* sizes, uint32_t* member_counts, int32_t cap"),
    "infx_engine_group_members_members": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap"),
    "infx_engine_group_members_totals": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total_groups, uint32_t* total"),
    "infx_engine_group_members_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_group_members_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* head_passes, uint32_t* hist_passes, "
                                             "uint32_t* member_walks, uint32_t* launches"),
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
    # the request structures, field for field: the device's is infx_group_list_req plus per_group
    grp = re.search(r"typedef struct infx_group_list_req \{([^}]*)\}", header("include/infidex_hip.h"))
    mem = re.search(r"typedef struct infx_group_members_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(mem.group(1).split()) == " ".join(grp.group(1).split()) + " uint32_t per_group; uint32_t reserved3;"
    m = re.search(r"typedef struct infx_group_members_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* group_by; const char* order_by; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t per_group;"
    assert [f[0] for f in E._GroupMembersReq._fields_] == ["filter", "group_by", "order_by", "ascending", "offset", "limit", "per_group"]
    h = header("include/infidex_hip.h")
    assert re.search(r"#define\s+INFX_GROUP_MEMBERS_MAX\s+4096\b", h) and re.search(r"#define\s+INFX_GROUP_MEMBERS_MAX_PER_GROUP\s+16\b", h)


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 8)()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_list_group_members(None, 0, None, None, None, None, None, None, None, None, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad group-members arguments"
    assert L.infx_last_group_members_stats(None, buf, buf, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_list_group_members(None, 0, None, None) == EINVAL
    assert L.infx_engine_group_members_rows(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_group_members_members(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_group_members_totals(None, 0, buf, buf) == EINVAL
    assert L.infx_engine_group_members_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_group_members_stats(None, buf, buf, buf, buf, buf, buf) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_list_group_members(sh, 1, None, None) == EINVAL                # requests announced, none given
    assert L.infx_engine_group_members_rows(sh, 0, None, None, None, 0) == -1           # nothing listed yet on this session
    assert L.infx_engine_group_members_members(sh, 0, None, None, None, 0) == -1
    assert L.infx_engine_group_members_totals(sh, 0, buf, buf) == EINVAL
    assert L.infx_engine_group_members_totals(sh, 0, None, buf) == EINVAL
    assert L.infx_engine_group_members_error(sh, 0, None, 0) == -1
    assert e.last_group_members_stats() == (0, 0, 0, 0, 0, 0)
    big = (E._GroupMembersReq * 17)()
    assert L.infx_engine_list_group_members(sh, 17, big, None) == ECAPACITY             # sixteen requests per call


def test_refusals_that_need_no_device_are_einval_of_their_own_request():
    """per_group, limits, offsets, group_by and order_by are checked per request before anything needs the device: on a host-only engine the call as a whole
    is INFX_EHIP, and the requests refused for one of them already carry INFX_EINVAL."""
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    R = E._GroupMembersReq
    reqs = [R(None, b"shade", None, 1, 0, 20, 0), R(None, b"shade", None, 1, 0, 20, 17), R(None, b"shade", None, 1, 0, 20, 1), R(None, b"shade", b"shade", 0, 0, 256, 16),
            R(None, b"shade", None, 1, 0, 241, 17), R(None, b"shade", None, 1, 0, 1024, 5), R(None, b"shade", None, 1, 0, 1024, 4), R(None, b"shade", None, 1, 0, 257, 16),
            R(None, b"shade", None, 1, 0, 0, 3), R(None, b"shade", None, 1, 0, 1025, 3), R(None, None, None, 1, 0, 20, 3), R(None, b"nosuch", None, 1, 0, 20, 3),
            R(None, b"shade", b"nosuch", 1, 0, 20, 3), R(None, b"shade", None, 1, 2 ** 31, 20, 3), R(b"shade = 'red'", b"shade", None, 1, 2 ** 31 - 1, 20, 3)]
    arr = (R * len(reqs))(*reqs)
    st = np.full(len(reqs), -7, np.int32)
    assert L.infx_engine_list_group_members(sh, len(reqs), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [EINVAL, EINVAL, 0, 0, EINVAL, EINVAL, 0, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, 0]
    buf = (C.c_uint32 * 4)()
    for which in range(len(reqs)):                                                      # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_group_members_rows(sh, which, None, None, None, 0) == -1
        assert L.infx_engine_group_members_members(sh, which, None, None, None, 0) == -1
        assert L.infx_engine_group_members_totals(sh, which, buf, buf) == EINVAL
        assert L.infx_engine_group_members_error(sh, which, None, 0) == -1


def test_host_only_engine_reports_ehip():
    e = host_engine()
    for args in ((None, "shade"), ("shade = 'red'", "shade", "shade", False, 16), ([GroupMembersRequest("shade = 'red'", "shade"), GroupMembersRequest(None, "shade", "shade", False, 2, 3, 5)],)):
        with pytest.raises(E.InfidexError) as ei:
            e.list_group_members(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                         # with a message
    assert e.last_group_members_stats() == (0, 0, 0, 0, 0, 0)


def test_field_names_and_defaults():
    r = GroupMembersRequest()
    assert [f for f in r.__dataclass_fields__] == ["filter", "group_by", "order_by", "ascending", "per_group", "offset", "limit"]
    assert (r.filter, r.group_by, r.order_by, r.ascending, r.per_group, r.offset, r.limit) == (None, None, None, True, 3, 0, 20)
    assert GroupMembersRequest("a = 1", "shop", "year", False, 5, 40, 10).limit == 10
    g = GroupMembers()
    assert [f for f in g.__dataclass_fields__] == ["group_value", "size", "document_ids", "values"]
    assert g.group_value == "" and g.size == 0 and g.document_ids == [] and g.values == []
    p = GroupMembersListing()
    assert [f for f in p.__dataclass_fields__] == ["groups", "total_groups", "total", "error"]
    assert p.groups == [] and p.total_groups == 0 and p.total == 0 and p.error is None
    want = [("filter", None), ("group_by", None), ("order_by", None), ("ascending", True), ("per_group", 3), ("offset", 0), ("limit", 20)]
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.list_group_members)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == want
        assert hasattr(owner, "last_group_members_stats")
    from infidex_amd.sharded import ShardedSearcher
    sig = inspect.signature(ShardedSearcher.list_group_members)
    assert [(k, v.default) for k, v in sig.parameters.items() if k != "self"] == want
    assert hasattr(ShardedSearcher, "last_group_members_stats")
    import infidex_amd
    assert {"GroupMembersListing", "GroupMembers", "GroupMembersRequest"} <= set(infidex_amd.__all__)
