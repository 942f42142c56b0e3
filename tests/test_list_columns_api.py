"""The C ABI and the Python surface of list columns without a GPU: the symbols are exported with the documented signatures, the arguments are checked before
anything is stored (mixed element kinds, a wrong document count, more list columns than the cap, a sharded engine), list columns and scalar columns share
one namespace in both directions, and a stored list comes back as it was given."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from infidex_amd import SearchEngine, LIB_PATH
from infidex_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EHIP, ECAPACITY, EUNSUPPORTED = 1, 3, 4, 5

SIGNATURES = {
    "infx_upload_list_column": ("include/infidex_hip.h", "int32_t", "infx_index* idx, uint32_t lcol, uint32_t total_docs, const uint32_t* elem_off, const uint32_t* elem_codes, uint32_t num_values"),
    "infx_list_leaf_build": ("include/infidex_hip.h", "int32_t", "infx_index* idx, uint32_t lcol, uint32_t k, const uint32_t* slots, const uint32_t* maps, uint32_t empty_bits"),
    "infx_list_facets": ("include/infidex_hip.h", "int32_t", "infx_stream* s, uint32_t lcol, uint32_t k, const uint8_t* const* masks, uint32_t* counts_out"),
    "infx_engine_add_list_column": ("include/infidex_engine.h", "int32_t", "infx_engine* e, const char* name, int32_t kind, int32_t facetable, int64_t n, const uint64_t* doc_offs, "
                                    "const int64_t* vals_i, const double* vals_d, const char* arena, const uint64_t* offs"),
    "infx_engine_list_column_count": ("include/infidex_engine.h", "int32_t", "infx_engine* e"),
    "infx_engine_list_column_info": ("include/infidex_engine.h", "int32_t", "infx_engine* e, int32_t lcol, char* name, int32_t cap, int32_t* facetable, int32_t* num_values, int32_t* kind"),
    "infx_engine_list_column_value": ("include/infidex_engine.h", "int32_t", "infx_engine* e, int32_t lcol, uint32_t code, char* out, int32_t cap"),
    "infx_engine_list_column_document": ("include/infidex_engine.h", "int64_t", "infx_engine* e, int32_t lcol, int64_t document_index, uint32_t* codes, int64_t cap"),
    "infx_engine_last_list_leaf_stats": ("include/infidex_engine.h", "int32_t", "infx_engine* e, uint32_t* built, uint32_t* launches"),
    "infx_engine_list_leaf_totals": ("include/infidex_engine.h", "int32_t", "infx_engine* e, uint64_t* built, uint64_t* launches"),
    "infx_engine_facets_all_list_column_count": ("include/infidex_engine.h", "int32_t", "infx_session* s"),
    "infx_engine_facets_all_list_column": ("include/infidex_engine.h", "int32_t", "infx_session* s, uint32_t k, int32_t* lcol, uint32_t* codes, uint32_t* counts, int32_t cap"),
    "infx_engine_facets_filtered_list_column_count": ("include/infidex_engine.h", "int32_t", "infx_session* s"),
    "infx_engine_facets_filtered_list_column": ("include/infidex_engine.h", "int32_t", "infx_session* s, uint32_t which, uint32_t k, int32_t* lcol, uint32_t* codes, uint32_t* counts, int32_t cap"),
}


def host_engine(n=3, shard=None):
    e = SearchEngine.create_default(device=-1, threads=1)
    if shard is not None:
        e._check(e.L.infx_engine_set_shard(e.h, shard[0], shard[1]))
    texts = [E._u16("alpha beta %d" % i) for i in range(n)]
    offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(t) for t in texts])
    e.index_flat(None, np.concatenate(texts), offs)
    return e


def header(name):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, name)).read(), flags=re.S)


def column_names(e):
    out = []
    for col in range(int(e.L.infx_engine_column_count(e.h))):
        nb = C.create_string_buffer(256); e.L.infx_engine_column_info(e.h, col, nb, 256, None, None)
        out.append(nb.value.decode())
    return out


def list_column_names(e):
    out = []
    for lcol in range(int(e.L.infx_engine_list_column_count(e.h))):
        nb = C.create_string_buffer(256); e.L.infx_engine_list_column_info(e.h, lcol, nb, 256, None, None, None)
        out.append(nb.value.decode())
    return out


def test_symbols_are_exported_with_the_documented_signatures():
    L = C.CDLL(LIB_PATH)
    for name, (hdr, ret, params) in SIGNATURES.items():
        assert getattr(L, name) is not None, name
        m = re.search(r"%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), header(hdr))
        assert m, name
        assert re.sub(r"\s*,\s*", ", ", " ".join(m.group(1).split())) == params, name
    h = header("include/infidex_engine.h"); d = header("include/infidex_hip.h")
    for text, name, value in ((h, "INFX_ENGINE_MAX_LIST_COLS", 8), (h, "INFX_ENGINE_MAX_LIST_FACETS", 4), (h, "INFX_ENGINE_MAX_DERIVED", 16),
                              (d, "INFX_MAX_LIST_COLS", 8), (d, "INFX_LIST_LEAF_MAX", 16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value, name


def test_null_and_bad_arguments_are_status_codes():
    L = C.CDLL(LIB_PATH)
    L.infx_engine_list_column_document.restype = C.c_int64
    buf = (C.c_uint32 * 4)(); offs = (C.c_uint64 * 4)(0, 1, 2, 3); vals = (C.c_int64 * 3)(1, 2, 3)
    assert L.infx_engine_add_list_column(None, b"t", 1, 0, C.c_int64(3), offs, vals, None, None, None) == EINVAL
    assert L.infx_upload_list_column(None, 0, 0, None, None, 0) == EINVAL
    assert L.infx_list_leaf_build(None, 0, 1, buf, buf, 0) == EINVAL
    assert L.infx_list_facets(None, 0, 1, None, buf) == EINVAL
    assert L.infx_engine_list_column_count(None) == -1
    assert L.infx_engine_last_list_leaf_stats(None, buf, buf) == EINVAL
    assert L.infx_engine_facets_all_list_column_count(None) == -1 and L.infx_engine_facets_filtered_list_column_count(None) == -1
    e = host_engine()
    add = lambda name, kind, n, o, v: L.infx_engine_add_list_column(e.h, name, kind, 0, C.c_int64(n), o, v, None, None, None)
    assert add(b"t", 0, 3, offs, vals) == EINVAL and add(b"t", 4, 3, offs, vals) == EINVAL          # kinds are 1, 2, 3
    assert add(b"", 1, 3, offs, vals) == EINVAL                                                    # a name
    assert add(b"t", 1, 2, offs, vals) == EINVAL                                                   # one list per indexed document
    assert add(b"t", 1, 3, None, vals) == EINVAL and add(b"t", 1, 3, offs, None) == EINVAL
    assert add(b"t", 1, 3, (C.c_uint64 * 4)(1, 1, 2, 3), vals) == EINVAL                           # offsets start at 0 ...
    assert add(b"t", 1, 3, (C.c_uint64 * 4)(0, 2, 1, 3), vals) == EINVAL                           # ... and ascend
    assert add(b"t", 1, 3, (C.c_uint64 * 4)(0, 1, 2, 2 ** 32), vals) == ECAPACITY                  # fewer than 2^32 elements
    assert L.infx_engine_list_column_count(e.h) == 0                                               # nothing was stored
    assert add(b"t", 1, 3, offs, vals) == 0
    assert L.infx_engine_list_column_info(e.h, 1, None, 0, None, None, None) == EINVAL
    assert L.infx_engine_list_column_value(e.h, 0, 3, None, 0) == -1
    assert L.infx_engine_list_column_document(e.h, 0, C.c_int64(3), None, C.c_int64(0)) == -1
    assert L.infx_engine_list_column_document(e.h, 1, C.c_int64(0), None, C.c_int64(0)) == -1
    assert e.last_list_leaf_stats() == (0, 0) and e.list_leaf_totals() == (0, 0)
    assert L.infx_engine_list_leaf_totals(None, None, None) == EINVAL
    assert L.infx_engine_add_column(e.h, b"", 1, 0, C.c_int64(3), vals, None, None, None) == EINVAL      # the nameless slot is the engine's own
    sh = e._default_session()
    assert L.infx_engine_facets_all_list_column(sh, 0, None, None, None, 0) == -1                  # nothing counted on this session
    assert L.infx_engine_facets_filtered_list_column(sh, 0, 0, None, None, None, 0) == -1


def test_mixed_kinds_and_a_wrong_document_count_raise_before_anything_is_stored():
    e = host_engine()
    for lists in ([[1], ["a"], []], [[1, 2.5], [], []], [[None], [], []], [[True], [], []], [[b"x"], [], []]):
        with pytest.raises(E.InfidexError) as ei:
            e.set_list_column("tags", lists)
        assert ei.value.code == EINVAL and "all int, or all float, or all str" in str(ei.value)
    for lists in ([[1], [2]], [[1], [2], [3], [4]], []):
        with pytest.raises(E.InfidexError) as ei:
            e.set_list_column("tags", lists)
        assert ei.value.code == EINVAL and "one list per indexed document" in str(ei.value)
    assert list_column_names(e) == []


def test_a_stored_list_comes_back_as_given():
    e = host_engine(4)
    e.set_list_column("tags", [["b", "a", "b", ""], [], ["ǆ", "B"], ("a",)], facetable=True)
    assert [e.list_column("tags", d) for d in range(4)] == [["b", "a", "b", ""], [], ["ǆ", "B"], ["a"]]
    e.set_list_column("nums", [[3, -1, 3], [2 ** 62], [], np.asarray([7, 7])])
    assert [e.list_column("nums", d) for d in range(4)] == [[3, -1, 3], [2 ** 62], [], [7, 7]]
    e.set_list_column("xs", [[0.5, -0.0], [1e300, float("inf")], [], [2.0]])
    got = [e.list_column("xs", d) for d in range(4)]
    assert got == [[0.5, -0.0], [1e300, float("inf")], [], [2.0]] and str(got[0][1]) == "-0.0"
    e.set_list_column("none", [[], [], [], []])
    assert [e.list_column("none", d) for d in range(4)] == [[], [], [], []]
    for bad in (-1, 4):
        with pytest.raises(E.InfidexError):
            e.list_column("tags", bad)
    with pytest.raises(E.InfidexError):
        e.list_column("nosuch", 0)
    # the dictionary follows encode_column: one code per distinct element, in order of first occurrence
    nv = C.c_int32(0); kind = C.c_int32(0); fac = C.c_int32(0)
    assert e.L.infx_engine_list_column_info(e.h, 0, None, 0, C.byref(fac), C.byref(nv), C.byref(kind)) == 0
    assert (fac.value, nv.value, kind.value) == (1, 5, 3)
    assert [E._list_column_value(e, 0, c) for c in range(5)] == ["b", "a", "", "ǆ", "B"]


def test_at_most_eight_list_columns_of_which_four_facetable():
    e = host_engine()
    for i in range(4):
        e.set_list_column("f%d" % i, [[i], [], []], facetable=True)
    with pytest.raises(E.InfidexError) as ei:
        e.set_list_column("f4", [[4], [], []], facetable=True)
    assert ei.value.code == ECAPACITY
    for i in range(4):
        e.set_list_column("p%d" % i, [[i], [], []])
    with pytest.raises(E.InfidexError) as ei:
        e.set_list_column("p4", [[4], [], []])
    assert ei.value.code == ECAPACITY
    with pytest.raises(E.InfidexError) as ei:
        e.set_list_column("p0", [[4], [], []], facetable=True)          # a fifth facetable one by replacement
    assert ei.value.code == ECAPACITY
    e.set_list_column("p0", [[9], [9], []])                             # replacing takes no new slot
    e.set_list_column("f0", [[9], [9], []], facetable=True)
    assert e.list_column("p0", 1) == [9] and sorted(list_column_names(e)) == sorted(["f%d" % i for i in range(4)] + ["p%d" % i for i in range(4)])
    # list columns take none of the 64 scalar slots
    for i in range(64):
        e.set_column("s%d" % i, np.arange(3))
    assert len(column_names(e)) == 64 and len(list_column_names(e)) == 8


def test_one_namespace_in_both_directions():
    e = host_engine()
    e.set_column("year", np.asarray([1999, 2000, 2001]))
    e.set_column("tags", ["a", "b", "c"], facetable=True)
    e.set_column("size", np.asarray([1.0, 2.0, 3.0]))
    # a list column takes a scalar column's name: the scalar column is gone, the slots of the others stay where they were
    e.set_list_column("tags", [["a", "b"], [], ["c"]])
    assert column_names(e) == ["year", "", "size"] and list_column_names(e) == ["tags"]
    assert E._column_index(e, "tags") == -1 and E._column_index(e, "size") == 2
    # a new scalar column takes the slot left behind
    e.set_column("shade", ["red", "red", "blue"])
    assert column_names(e) == ["year", "shade", "size"]
    # a scalar column takes a list column's name: the list column is gone and its slot is free for the next one
    e.set_column("tags", ["x", "y", "z"])
    assert column_names(e) == ["year", "shade", "size", "tags"] and list_column_names(e) == [""]
    with pytest.raises(E.InfidexError):
        e.list_column("tags", 0)
    e.set_list_column("genres", [["g"], [], []])
    assert list_column_names(e) == ["genres"] and e.list_column("genres", 0) == ["g"]
    # a list column replaces a list column of its name, of another kind
    e.set_list_column("genres", [[1, 2], [3], []])
    assert list_column_names(e) == ["genres"] and e.list_column("genres", 0) == [1, 2]


def test_a_sharded_engine_refuses_list_columns():
    e = host_engine(shard=(0, 2))
    with pytest.raises(E.InfidexError) as ei:
        e.set_list_column("tags", [["a"], [], []])
    assert ei.value.code == EUNSUPPORTED and "sharded" in str(ei.value)
    assert list_column_names(e) == []
    e.set_column("tags", ["a", "b", "c"])                              # scalar columns are what they were


def test_filters_and_facets_need_the_device():
    e = host_engine()
    e.set_list_column("tags", [["a"], [], ["b"]], facetable=True)
    with pytest.raises(E.InfidexError) as ei:
        e.facets_of_documents("tags = 'a'")
    assert ei.value.code == EHIP
    with pytest.raises(E.InfidexError) as ei:
        e.facets_of_all_documents()
    assert ei.value.code == EHIP
    with pytest.raises(E.InfidexError) as ei:
        e.list_documents("tags = 'a'")
    assert ei.value.code == EHIP
