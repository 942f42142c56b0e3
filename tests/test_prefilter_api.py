"""Query.pre_filter: the public surface that needs no GPU — the dataclass fields, the exported symbols and their header declarations, the helper that
splits a batch so that no device batch carries more than 16 distinct pre-filters, and the unchanged layout of infx_query_options."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np

from infidex_amd import Query, Result, load_library, MAX_PREFILTERS
from infidex_amd.engine import _QueryOptions, _by_depth, _split_prefilters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_SYMBOLS = ["infx_engine_set_query_prefilters", "infx_engine_last_in_prefilter", "infx_engine_last_prefilter_stats", "infx_engine_prefilter_mask"]
DEVICE_SYMBOLS = ["infx_filter_masks", "infx_stream_set_doc_masks", "infx_stream_mask_slot", "infx_last_filter_mask_stats"]


def test_query_and_result_fields():
    assert Query("x").pre_filter is None
    assert Query("x", pre_filter="year > 2000").pre_filter == "year > 2000"
    names = [f.name for f in dataclasses.fields(Result)]
    assert names[-1] == "error" and names[-2] == "total_in_pre_filter"
    r = Result()
    assert r.total_in_pre_filter == 0 and r.error is None
    # positional construction up to total_in_filter is what existing callers use: the new field sits behind it
    assert names.index("total_in_filter") == names.index("total_in_pre_filter") - 1


def test_symbols_are_exported_and_declared():
    L = load_library()
    hdr = {"infidex_engine.h": ENGINE_SYMBOLS, "infidex_hip.h": DEVICE_SYMBOLS}
    for h, syms in hdr.items():
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for s in syms:
            assert hasattr(L, s), s
            assert re.search(r"\bint32_t\s+%s\s*\(" % s, src), (h, s)
    src = open(os.path.join(ROOT, "include", "infidex_hip.h")).read()
    m = re.search(r"#define\s+INFX_MAX_PREFILTERS\s+(\d+)", src)
    assert m and int(m.group(1)) == MAX_PREFILTERS == 16


def test_null_session_is_refused():
    L = load_library()
    assert L.infx_engine_set_query_prefilters(None, 0, None, None) != 0
    assert L.infx_engine_last_in_prefilter(None, 0, None) != 0
    assert L.infx_engine_last_prefilter_stats(None, None, None, None) != 0
    assert L.infx_engine_prefilter_mask(None, None, None, C.c_uint64(0)) != 0
    assert L.infx_filter_masks(None, 0, None, None, None) != 0
    assert L.infx_stream_set_doc_masks(None, 0, None) != 0
    assert L.infx_stream_mask_slot(None, 0, None) != 0


def _groups(qs, limit=MAX_PREFILTERS):
    return _split_prefilters(qs, _by_depth(qs), limit)


def test_split_keeps_order_and_bounds_the_distinct_expressions():
    rng = np.random.default_rng(3)
    for trial in range(20):
        n = int(rng.integers(1, 200))
        nexpr = int(rng.integers(1, 60))
        qs = [Query("q%d" % i, coverage_depth=int(rng.choice([100, 500])),
                    pre_filter=None if rng.random() < 0.3 else "year > %d" % int(rng.integers(nexpr))) for i in range(n)]
        groups = _groups(qs)
        seen = []
        for depth, idx in groups:
            assert idx == sorted(idx) and idx
            assert all(qs[i].coverage_depth == depth for i in idx)
            assert len({qs[i].pre_filter for i in idx if qs[i].pre_filter is not None}) <= 16
            seen += idx
        assert sorted(seen) == list(range(n))                      # every query once
        for depth in {q.coverage_depth for q in qs}:               # input order inside a depth, across its groups
            flat = [i for d, idx in groups if d == depth for i in idx]
            assert flat == [i for i in range(n) if qs[i].coverage_depth == depth]


def test_split_leaves_small_batches_alone():
    qs = [Query("a", pre_filter="year > %d" % (i % 16)) for i in range(64)] + [Query("b")] * 5
    assert _groups(qs) == _by_depth(qs)                            # 16 distinct expressions: one batch
    qs17 = [Query("a", pre_filter="year > %d" % i) for i in range(17)]
    g = _groups(qs17)
    assert [idx for _, idx in g] == [list(range(16)), [16]]
    assert _groups([Query("a"), Query("b")]) == _by_depth([Query("a"), Query("b")])
    # a repeated expression after the limit stays in the group that already holds it
    qs = [Query("a", pre_filter="year > %d" % i) for i in range(16)] + [Query("a", pre_filter="year > 3"), Query("a", pre_filter="year > 99")]
    assert [idx for _, idx in _groups(qs)] == [list(range(17)), [17]]


def test_query_options_layout_is_unchanged():
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(_QueryOptions) == 16 + 6 * p
    assert [f[0] for f in _QueryOptions._fields_] == ["max_results", "enable_coverage", "enable_facets", "enable_boost", "filter", "nboosts", "boost_filters",
                                                      "boost_strengths", "sort_by", "sort_ascending"]
