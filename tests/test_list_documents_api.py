"""The C ABI and the Python surface of list_documents (a filter's documents in the order of a field, by page) without a GPU: the symbols are exported with
the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (the selection has no CPU fallback), limits and digit widths
out of range are INFX_EINVAL, and Listing / ListRequest default to "everything, index order, first page of 20"."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, Listing, ListRequest, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_list_ordered": ("include/infidex_hip.h", "infx_stream* s, uint32_t nreq, const infx_list_req* reqs, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out, "
                          "uint32_t* counts_out, uint32_t* totals_out"),
    "infx_last_list_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t* hist_passes, uint32_t* launches"),
    "infx_engine_list_documents": ("include/infidex_engine.h", "infx_session* s, uint32_t nreq, const infx_list_request* reqs, int32_t* out_status"),
    "infx_engine_list_rows": ("include/infidex_engine.h", "infx_session* s, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap"),
    "infx_engine_list_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_list_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_list_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* hist_passes, uint32_t* launches"),
    "infx_engine_set_list_digit_bits": ("include/infidex_engine.h", "infx_session* s, int32_t bits"),
}
EINVAL, EHIP = 1, 3


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    a = E._u16("alpha beta gamma"); offs = np.asarray([0, len(a)], np.uint64)
    e.index_flat(None, a, offs)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header(hdr))
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)
    # the request structures, field for field
    m = re.search(r"typedef struct infx_list_req \{([^}]*)\}", header("include/infidex_hip.h"))
    assert " ".join(m.group(1).split()) == "const uint8_t* mask; int32_t col; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t digit_bits; uint32_t reserved;"
    m = re.search(r"typedef struct infx_list_request \{([^}]*)\}", header("include/infidex_engine.h"))
    assert " ".join(m.group(1).split()) == "const char* filter; const char* order_by; int32_t ascending; uint32_t offset; uint32_t limit;"
    assert [f[0] for f in E._ListReq._fields_] == ["filter", "order_by", "ascending", "offset", "limit"]


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)()
    L.infx_last_error.restype = C.c_char_p
    assert L.infx_list_ordered(None, 0, None, None, None, None, None, None) == EINVAL
    assert L.infx_last_error() == b"bad listing arguments"
    assert L.infx_last_list_stats(None, buf, buf) == EINVAL
    assert L.infx_last_error() == b"null argument"
    assert L.infx_engine_list_documents(None, 0, None, None) == EINVAL
    assert L.infx_engine_list_rows(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_list_total(None, 0, buf) == EINVAL
    assert L.infx_engine_list_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_list_stats(None, buf, buf, buf, buf) == EINVAL
    assert L.infx_engine_set_list_digit_bits(None, 11) == EINVAL
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_list_documents(sh, 1, None, None) == EINVAL                  # requests announced, none given
    assert L.infx_engine_list_rows(sh, 0, None, None, None, 0) == -1                  # nothing listed yet on this session
    assert L.infx_engine_list_total(sh, 0, buf) == EINVAL
    assert L.infx_engine_list_error(sh, 0, None, 0) == -1
    assert e.last_list_stats() == (0, 0, 0, 0)


def test_digit_bits_outside_4_to_11_are_einval():
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    for bits, rc in ((3, EINVAL), (12, EINVAL), (0, EINVAL), (-1, EINVAL), (4, 0), (5, 0), (11, 0)):
        assert L.infx_engine_set_list_digit_bits(sh, bits) == rc, bits
    with pytest.raises(E.InfidexError) as ei:
        e.set_list_digit_bits(12)
    assert ei.value.code == EINVAL
    e.set_list_digit_bits(11)


def test_limits_outside_1_to_1024_are_einval_of_their_own_request():
    """The limit is checked per request before anything needs the device: on a host-only engine the call as a whole is INFX_EHIP, and the requests whose
    limit or offset is out of range already carry INFX_EINVAL."""
    L = C.CDLL(LIB_PATH)
    e = host_engine()
    sh = e._default_session()
    limits = [0, 1025, 1, 1024, 20]
    arr = (E._ListReq * len(limits))()
    for i, lim in enumerate(limits):
        arr[i] = E._ListReq(None, None, 1, 0, lim)
    st = np.full(len(limits), -7, np.int32)
    assert L.infx_engine_list_documents(sh, len(limits), arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP
    assert st.tolist() == [EINVAL, EINVAL, 0, 0, 0]
    buf = (C.c_uint32 * 4)()
    for which in range(len(limits)):                                                  # a call that failed as a whole leaves no answers for the readers
        assert L.infx_engine_list_rows(sh, which, None, None, None, 0) == -1
        assert L.infx_engine_list_total(sh, which, buf) == EINVAL
        assert L.infx_engine_list_error(sh, which, None, 0) == -1
    arr[0] = E._ListReq(None, None, 1, 2 ** 31, 20)                                   # offsets stop below 2^31
    assert L.infx_engine_list_documents(sh, 1, arr, st.ctypes.data_as(C.POINTER(C.c_int32))) == EHIP and st[0] == EINVAL
    big = (E._ListReq * 17)()
    assert L.infx_engine_list_documents(sh, 17, big, None) == 4                       # INFX_ECAPACITY: sixteen requests per call


def test_host_only_engine_reports_ehip():
    e = host_engine()
    e.set_column("shade", ["red"], facetable=True)
    for args in ((), ("shade = 'red'", "shade"), ([ListRequest("shade = 'red'"), ListRequest(None, "shade", False, 3, 5)],)):
        with pytest.raises(E.InfidexError) as ei:
            e.list_documents(*args)
        assert ei.value.code == EHIP and "GPU" in str(ei.value)                       # with a message
    assert e.last_list_stats() == (0, 0, 0, 0)


def test_defaults():
    r = ListRequest()
    assert (r.filter, r.order_by, r.ascending, r.offset, r.limit) == (None, None, True, 0, 20)
    assert ListRequest("a = 1", "year", False, 40, 10).limit == 10
    p = Listing()
    assert p.document_ids == [] and p.values == [] and p.total == 0 and p.error is None
    import inspect
    for owner in (SearchEngine, E.Session):
        sig = inspect.signature(owner.list_documents)
        assert [(k, v.default) for k, v in sig.parameters.items() if k not in ("self", "session")] == \
            [("filter", None), ("order_by", None), ("ascending", True), ("offset", 0), ("limit", 20)]
    from infidex_amd.sharded import ShardedSearcher
    assert list(inspect.signature(ShardedSearcher.list_documents).parameters)[1:] == ["filter", "order_by", "ascending", "offset", "limit"]
