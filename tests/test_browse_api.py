"""The C ABI of the browse rows and the whole-corpus facets without a GPU: the symbols are exported, their arguments are checked, and a host-only
engine answers INFX_EHIP (these paths have no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from infidex_amd import SearchEngine, Query, LIB_PATH
from infidex_amd import engine as E

NEW_SYMBOLS = ["infx_set_first_live", "infx_last_browse_stats", "infx_facets_all", "infx_engine_facets_all", "infx_engine_facets_all_column",
               "infx_engine_delete_document_ids", "infx_engine_last_browse_stats"]


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    a = E._u16("alpha beta gamma"); offs = np.asarray([0, len(a)], np.uint64)
    e.index_flat(None, a, offs)
    return e


def test_symbols_are_exported():
    L = C.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None, name


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)()
    assert L.infx_set_first_live(None, 0, None) == 1                     # INFX_EINVAL
    assert L.infx_last_browse_stats(None, buf, buf) == 1
    assert L.infx_facets_all(None, 0, None, None) == 1
    assert L.infx_engine_facets_all(None, None) == 1
    assert L.infx_engine_facets_all_column(None, 0, None, None, None, 0) == -1
    assert L.infx_engine_delete_document_ids(None, None, C.c_int64(0), None) == 1
    e = host_engine()
    assert L.infx_engine_delete_document_ids(e.h, None, C.c_int64(3), None) == 1
    sh = e._default_session()
    assert L.infx_engine_facets_all_column(sh, 0, None, None, None, 0) == -1      # nothing counted yet on this session


def test_host_only_engine_reports_ehip():
    e = host_engine()
    e.set_column("shade", ["red"], facetable=True)
    with pytest.raises(E.InfidexError) as ei:
        e.facets_of_all_documents()
    assert ei.value.code == 3 and "GPU" in str(ei.value)                 # INFX_EHIP
    with pytest.raises(E.InfidexError) as ei:
        e.search(Query("", 10, enable_facets=True))                      # a browse query runs on the device like any other
    assert ei.value.code == 3
    with pytest.raises(E.InfidexError) as ei:
        e.search_queries([Query("", 10, filter="shade = 'red'", enable_facets=True)])
    assert ei.value.code == 3
    assert e.delete_document_ids([0, 7, -1]) == 1                        # host state only: ids out of range are ignored
    assert e.delete_document_ids([0]) == 0
    e.restore_documents()
