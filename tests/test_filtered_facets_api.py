"""The C ABI and the Python surface of the filtered facets (facets of the documents a filter accepts) without a GPU: the symbols are exported with
the documented signatures, their arguments are checked, a host-only engine answers INFX_EHIP (the counting has no CPU fallback), and the new
Query / Result members default to "off"."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, Query, Result, FilteredFacets, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the parameter list the headers document (whitespace and comments normalised)
SIGNATURES = {
    "infx_facets_filtered": ("include/infidex_hip.h", "infx_stream* s, uint32_t k, const infx_filter_prog* progs, uint32_t ncol, const uint32_t* cols, "
                             "uint32_t* counts_out, uint32_t* totals_out"),
    "infx_last_facets_filtered_stats": ("include/infidex_hip.h", "infx_stream* s, uint32_t* programs, uint32_t* launches"),
    "infx_engine_facets_filtered": ("include/infidex_engine.h", "infx_session* s, uint32_t k, const char* const* exprs, int32_t* out_status"),
    "infx_engine_facets_filtered_column_count": ("include/infidex_engine.h", "infx_session* s"),
    "infx_engine_facets_filtered_column": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap"),
    "infx_engine_facets_filtered_total": ("include/infidex_engine.h", "infx_session* s, uint32_t which, uint32_t* total"),
    "infx_engine_facets_filtered_error": ("include/infidex_engine.h", "infx_session* s, uint32_t which, char* out, int32_t cap"),
    "infx_engine_last_facets_filtered_stats": ("include/infidex_engine.h", "infx_session* s, uint32_t* counted, uint32_t* cached, uint32_t* launches"),
}


def host_engine():
    e = SearchEngine.create_default(device=-1, threads=1)
    a = E._u16("alpha beta gamma"); offs = np.asarray([0, len(a)], np.uint64)
    e.index_flat(None, a, offs)
    return e


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (header, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, header)).read(), flags=re.S)
        m = re.search(r"int32_t\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        got = re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split()))
        assert got == params, (name, got)


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    buf = (C.c_uint32 * 4)()
    assert L.infx_facets_filtered(None, 0, None, 0, None, None, None) == 1            # INFX_EINVAL
    assert L.infx_last_facets_filtered_stats(None, buf, buf) == 1
    assert L.infx_engine_facets_filtered(None, 0, None, None) == 1
    assert L.infx_engine_facets_filtered_column_count(None) == -1
    assert L.infx_engine_facets_filtered_column(None, 0, 0, None, None, None, 0) == -1
    assert L.infx_engine_facets_filtered_total(None, 0, buf) == 1
    assert L.infx_engine_facets_filtered_error(None, 0, None, 0) == -1
    assert L.infx_engine_last_facets_filtered_stats(None, buf, buf, buf) == 1
    e = host_engine()
    sh = e._default_session()
    assert L.infx_engine_facets_filtered_column(sh, 0, 0, None, None, None, 0) == -1  # nothing counted yet on this session
    assert L.infx_engine_facets_filtered_total(sh, 0, buf) == 1
    assert L.infx_engine_facets_filtered_error(sh, 0, None, 0) == -1
    assert e.last_filtered_facet_stats() == (0, 0, 0)


def test_host_only_engine_reports_ehip():
    e = host_engine()
    e.set_column("shade", ["red"], facetable=True)
    for arg in ("shade = 'red'", ["shade = 'red'", "shade = 'blue'"]):
        with pytest.raises(E.InfidexError) as ei:
            e.facets_of_documents(arg)
        assert ei.value.code == 3 and "GPU" in str(ei.value)                          # INFX_EHIP, with a message
    with pytest.raises(E.InfidexError) as ei:
        e.search(Query("alpha", 10, pre_filter="shade = 'red'", pre_filter_facets=True))
    assert ei.value.code == 3


def test_defaults():
    q = Query("x")
    assert q.pre_filter_facets is False and q.pre_filter is None
    r = Result()
    assert r.pre_filter_facets is None and r.facets is None and r.total_in_pre_filter == 0
    f = FilteredFacets()
    assert f.facets == {} and f.total == 0 and f.error is None
    assert Query("x", pre_filter="a = 1", pre_filter_facets=True).pre_filter_facets is True
