"""The four per-query setting calls of a session (options, coverage setups, pre-filters, collapse requests) as ONE frame, without a GPU: on a host-only
engine the coverage and collapse installers work, so two parts of one batch show the message rule of infx_engine_query_error (per query the first message
among the installed parts in the fixed order options, coverage, pre-filters, collapse, whichever was installed last; "" for a query none refuses), a part
installed alone forgets the batch before it, a search of another size names the part it clears, and the null / clear forms of both installers."""
import ctypes as C

import numpy as np
import pytest

from infidex_amd import CoverageSetup
from infidex_amd.engine import _CoverageSetup, _coverage_struct, _p, pack_texts
from tests.test_collapse_api import host_engine

EINVAL, EUNSUPPORTED = 1, 5


def install_coverage(e, sh, setups, status=True):
    n = len(setups)
    sts = [_coverage_struct(s) if s is not None else None for s in setups]
    ptrs = (C.POINTER(_CoverageSetup) * max(n, 1))(*[C.pointer(s) if s is not None else None for s in sts])
    st = np.full(max(n, 1), -7, np.int32)
    assert e.L.infx_engine_set_query_coverage(sh, n, ptrs, _p(st, C.c_int32) if status else None) == 0
    return st[:n].tolist()


def install_collapse(e, sh, fields, keeps, status=True):
    n = len(fields)
    names = (C.c_char_p * max(n, 1))(*fields); ks = (C.c_int32 * max(n, 1))(*keeps)
    st = np.full(max(n, 1), -7, np.int32)
    assert e.L.infx_engine_set_query_collapse(sh, n, names, ks, _p(st, C.c_int32) if status else None) == 0
    return st[:n].tolist()


def messages(e, sh, n):
    buf = C.create_string_buffer(512); out = []
    for i in range(n):
        assert e.L.infx_engine_query_error(sh, i, buf, 512) == len(buf.value)
        out.append(buf.value.decode())
    return out


SETUPS = [None, CoverageSetup(enable_lexical_prescreen=True), CoverageSetup(truncate=False), CoverageSetup(truncation_score=999)]
FIELDS, KEEPS = [None, b"nosuch", b"shade", None], [1, 1, 0, 1]


@pytest.mark.parametrize("coverage_first", [True, False])
def test_two_parts_of_one_batch_share_the_messages_in_the_fixed_order(coverage_first):
    e = host_engine(); sh = e._default_session()
    if coverage_first:
        cst = install_coverage(e, sh, SETUPS); kst = install_collapse(e, sh, FIELDS, KEEPS)
    else:
        kst = install_collapse(e, sh, FIELDS, KEEPS); cst = install_coverage(e, sh, SETUPS)
    assert cst == [0, EUNSUPPORTED, 0, EINVAL]          # each call's statuses are its own part's
    assert kst == [0, EINVAL, EINVAL, 0]
    m = messages(e, sh, 4)
    assert m[0] == ""
    assert "LexicalPrescreen" in m[1]                    # refused by both: coverage comes before collapse
    assert "collapse_keep" in m[2]
    assert "TruncationScore" in m[3]
    assert e.L.infx_engine_query_error(sh, 4, C.create_string_buffer(8), 8) == -1


def test_a_part_alone_forgets_the_last_batch():
    e = host_engine(); sh = e._default_session()
    assert install_collapse(e, sh, FIELDS, KEEPS) == [0, EINVAL, EINVAL, 0]
    assert "collapse_keep" in messages(e, sh, 4)[2]
    assert install_collapse(e, sh, [], []) == []        # nq = 0 clears
    assert install_coverage(e, sh, [None] * 4) == [0, 0, 0, 0]
    # "One frame behind the session's four per-query setting calls", allowed difference 1: before it the coverage installer alone left query 1's and
    # query 2's messages of the batch above in place
    assert messages(e, sh, 4) == [""] * 4


@pytest.mark.parametrize("part, text", [("collapse", "collapse requests"), ("coverage", "coverage setups")])
def test_a_search_of_another_size_fails_and_names_the_part(part, text):
    e = host_engine(); sh = e._default_session()
    if part == "collapse":
        install_collapse(e, sh, [b"shade", None, None], [1, 1, 1])
    else:
        install_coverage(e, sh, [None, CoverageSetup(truncate=False), None])
    arena, offs = pack_texts(["alpha", "beta"])
    keys = np.full((2, 4), -1, np.int64); scores = np.zeros((2, 4), np.float32); counts = np.zeros(2, np.uint32)
    rc = e.L.infx_engine_search_batch(e.h, 2, _p(arena, C.c_uint16), _p(offs, C.c_uint64), 4, 500, 1, _p(keys, C.c_int64), _p(scores, C.c_float), None,
                                      _p(counts, C.c_uint32), None)
    assert rc == EINVAL
    assert (text + " were installed for a batch of another size") in e.L.infx_engine_last_error().decode()


@pytest.mark.parametrize("part", ["coverage", "collapse"])
def test_null_and_clear_forms(part):
    e = host_engine(); sh = e._default_session(); L = e.L
    if part == "coverage":
        call = lambda s, n, a, st: L.infx_engine_set_query_coverage(s, n, a, st)
        one = (C.POINTER(_CoverageSetup) * 1)(C.pointer(_coverage_struct(CoverageSetup(truncate=False))))
    else:
        keeps = (C.c_int32 * 1)(1)
        call = lambda s, n, a, st: L.infx_engine_set_query_collapse(s, n, a, keeps if a is not None else None, st)
        one = (C.c_char_p * 1)(b"nosuch")
    assert call(sh, 0, None, None) == 0                  # nq = 0 clears, with nothing installed too
    assert call(None, 1, one, None) == EINVAL            # a NULL session
    assert call(None, 0, None, None) == EINVAL
    assert call(sh, 1, one, None) == 0                   # out_status may be NULL
    assert call(sh, 0, None, None) == 0
