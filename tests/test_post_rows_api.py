"""SearchEngine(max_post_rows=...) / infx_engine_set_post_rows / infx_set_post_rows without a GPU: the range, the default, the pass-through of the
constructors and the NULL handles.  What the setting does on the device is tests/test_gpu_post_rows.py's."""
import ctypes as C

import pytest

from infidex_amd import SearchEngine, LIB_PATH
from infidex_amd.engine import InfidexError


def test_default_range_and_pass_through():
    e = SearchEngine.create_default(device=-1, threads=1)
    assert e.max_post_rows == 64
    for v in (64, 65, 300, 1024):
        assert e.L.infx_engine_set_post_rows(e.h, v) == 0 and e.max_post_rows == v
    for v in (63, 1025, 0, -5):
        assert e.L.infx_engine_set_post_rows(e.h, v) == 1 and e.max_post_rows == 1024        # INFX_EINVAL, the value stays
        assert b"64" in e.L.infx_engine_last_error() and b"1024" in e.L.infx_engine_last_error()
    e.close()
    for make in (SearchEngine, SearchEngine.create_default, SearchEngine.create_minimal):
        x = make(device=-1, threads=1, max_post_rows=300)
        assert x.max_post_rows == 300
        x.close()
        for bad in (63, 1025, 2 ** 40):
            with pytest.raises(InfidexError) as ei:
                make(device=-1, threads=1, max_post_rows=bad)
            assert ei.value.code == 1


def test_null_handles_and_constants():
    L = C.CDLL(LIB_PATH)
    out = C.c_int32(7)
    assert L.infx_engine_set_post_rows(None, 128) == 1 and L.infx_engine_get_post_rows(None, C.byref(out)) == 1
    assert L.infx_set_post_rows(None, 128) == 1 and L.infx_get_post_rows(None, C.byref(out)) == 1 and out.value == 7
    hdr = open(LIB_PATH.rsplit("/infidex_amd/", 1)[0] + "/include/infidex_hip.h").read()
    assert "#define INFX_FILTER_MAX_ROWS 64 " in hdr and "#define INFX_POST_MAX_ROWS 1024 " in hdr
