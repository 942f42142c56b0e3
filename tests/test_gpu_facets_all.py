"""SearchEngine.facets_of_all_documents on the GPU (FacetBuilder.BuildFacetsFromAllDocuments, Core/FacetBuilder.cs:110-181) against plain counting
(tests/browse_model.py): value counts of every facetable column over all live documents, per document; null / empty values left out; count
descending then value ascending; at most 100 values per field; fields without a value absent.  The columns cover the kernel's two counting paths
(per-workgroup LDS counters for small dictionaries, global counters for large ones) and the cut at 100 among equal counts."""
import numpy as np
import pytest

from infidex_amd import SearchEngine
from tests.browse_model import BrowseModel
from tools.synth import Synth

pytestmark = pytest.mark.gpu

D = 70000


@pytest.fixture(scope="module")
def fx():
    s = Synth(2, docs=D)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    rng = np.random.default_rng(11)
    ten = ["c%d" % v for v in rng.integers(0, 10, D)]                              # 10 values (same-case ASCII + digits: ordinal == culture order)
    # 130 values: v100..v189 occur exactly 300 times each (equal counts around rank 100: the cut falls inside a tie), v190..v229 more often
    many = np.concatenate([np.repeat(np.arange(100, 190), 300), rng.integers(190, 230, D - 90 * 300)])
    rng.shuffle(many)
    many = ["v%d" % v for v in many]
    wide = rng.permutation(np.arange(D, dtype=np.int64) % 55000 + 100000)         # 55 000 distinct values of equal width, 15 000 of them twice
    holes = [("" if v % 3 == 0 else "h%d" % (v % 7)) for v in rng.integers(0, 1000, D)]   # a third of the documents have no value
    empty = [""] * D                                                               # a facetable field without any value: absent
    hidden = ["x%d" % (v % 5) for v in range(D)]                                   # not facetable
    cols = {"ten": (ten, True), "many": (many, True), "wide": (wide, True), "holes": (holes, True), "empty": (empty, True), "hidden": (hidden, False)}
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    assert len(set(wide.tolist())) >= 50000
    return e, BrowseModel(cols)


def test_all_documents(fx):
    e, m = fx
    got = e.facets_of_all_documents()
    want = m.all_facets()
    assert set(got) == {"ten", "many", "wide", "holes"}
    assert got == want
    assert len(got["many"]) == 100 and len(got["wide"]) == 100 and len(got["ten"]) == 10
    assert got["many"][99][1] == 300 and got["many"][40][1] == 300                 # the cut falls among the values that occur 300 times
    assert sum(c for _, c in got["ten"]) == D
    assert all(v for v, _ in got["holes"])


def test_after_deletions_and_restore(fx):
    e, m = fx
    gone = list(range(0, D, 7)) + [D - 1]
    gone = sorted(set(gone))
    try:
        assert e.delete_documents(gone) == len(gone)
        m.deleted = set(gone)
        got = e.facets_of_all_documents()
        assert got == m.all_facets()
        assert sum(c for _, c in got["ten"]) == D - len(gone)
    finally:
        e.restore_documents(); m.deleted = set()
    assert e.facets_of_all_documents() == m.all_facets()


def test_two_calls_agree_and_sessions_share_nothing(fx):
    e, m = fx
    from infidex_amd.engine import Session
    s = Session(e)
    try:
        assert s.facets_of_all_documents() == e.facets_of_all_documents() == e.facets_of_all_documents()
    finally:
        s.close()


def test_small_dictionaries_beyond_the_lds_budget_use_global_counters():
    """Five columns of 4000 values each: every one is small enough for per-workgroup LDS counters, but together they exceed the 16 384 words the
    kernel allows itself, so the last one is counted in global memory although its dictionary is small.  (A sixth, tiny column fits again.)"""
    n = 30000
    s = Synth(2, docs=n)
    arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    rng = np.random.default_rng(17)
    cols = {}
    for k in range(5):
        cols["f%d" % k] = (["w%04d" % v for v in rng.integers(0, 4000, n)], True)
    cols["tiny"] = (["t%d" % v for v in rng.integers(0, 3, n)], True)
    for name, (vals, fac) in cols.items():
        e.set_column(name, vals, facetable=fac)
    m = BrowseModel(cols)
    got = e.facets_of_all_documents()
    assert got == m.all_facets()
    assert set(got) == set(cols) and all(len(got["f%d" % k]) == 100 for k in range(5)) and sum(c for _, c in got["tiny"]) == n
    gone = list(range(5, n, 11))
    assert e.delete_documents(gone) == len(gone)
    m.deleted = set(gone)
    assert e.facets_of_all_documents() == m.all_facets()
