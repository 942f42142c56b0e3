"""Python surface of the per-query options (no GPU): the Result field, the CoverageDepth grouping and the ctypes mirror of infx_query_options."""
import ctypes as C
import dataclasses

from infidex_amd import Query, Result, Boost
from infidex_amd.engine import _QueryOptions, _by_depth


def test_result_error_is_the_last_field():
    assert [f.name for f in dataclasses.fields(Result)][-1] == "error"
    assert Result().error is None


def test_batches_group_by_coverage_depth_in_input_order():
    qs = [Query("a", coverage_depth=500), Query("b", coverage_depth=100), Query("c", coverage_depth=500), Query("d", coverage_depth=100)]
    assert _by_depth(qs) == [(500, [0, 2]), (100, [1, 3])]


def test_query_options_layout():
    # int32 x4, char*, uint32, char**, int32*, char*, int32 (include/infidex_engine.h)
    p = C.sizeof(C.c_void_p)
    assert _QueryOptions.filter.offset == 16 and _QueryOptions.nboosts.offset == 16 + p
    assert _QueryOptions.boost_filters.offset == 16 + 2 * p and _QueryOptions.sort_by.offset == 16 + 4 * p
    assert C.sizeof(_QueryOptions) == 16 + 6 * p
    assert Query("x", enable_boost=True, boosts=[Boost("a = 1", 3)]).max_boost == 3
