"""The sixteen-document set walk (infidex_amd/csrc/set_walk.h) on the GPU, at the shapes at which a reader of the partial last group once went wrong, on every
feature that walks: list_documents, range_facets and field_stats (list_groups walks them in tests/test_gpu_list_groups.py, whose corpora and filters these are).

Corpora of 12, 13, 14, 15, 17 and 31 documents: less than two groups of 16, so the flags of the partial last group are read one by one.  The filters leave
every run of accepted documents that begins or ends inside a group of four (1111 1000 0000: the first of a four alone refused), `size = 5`, two runs, and no
filter.  Per filter: list_documents by `size` ascending, by `shade` descending and in index order against ListModel; range_facets over `size` with edges at 1, 5,
9 and n + 1 and field_stats of `size`, whole and grouped by `shade`, against counts taken with numpy over the documents ListModel accepts.  Every comparison is
exact equality."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, ListRequest
from infidex_amd.engine import RangeRequest, StatsRequest
from tests.test_gpu_list_documents import ListModel, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [12, 13, 14, 15, 17, 31])
def test_small_corpora_every_shape_of_the_partial_last_group_on_every_walk(n):
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    shade = (["red", "blue", "green"] * 11)[:n]
    size = np.arange(1, n + 1, dtype=np.int64)
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(n)])
    e.set_column("shade", shade, facetable=True); e.set_column("size", size, facetable=False)
    lm = ListModel({"shade": (shade, True), "size": (size, False)}, list(range(100, 100 + n)))
    filters = ["size >= %d" % v for v in range(1, n + 2)] + ["size <= %d" % v for v in range(1, n)] + ["size = 5", "size = 6 OR size = 11", "size = 9 OR size >= 13", None]
    members = {x: lm.order(x, None, True) for x in filters}                  # the accepted documents, ascending
    assert len(members["size >= %d" % (n + 1)]) == 0 and len(members[None]) == n and list(members["size = 6 OR size = 11"]) == [5, 10]

    run(e, lm, [ListRequest(x, c, asc, 0, 40) for x in filters for c, asc in (("size", True), ("shade", False), (None, True))], n)

    edges = (1, 5, 9, n + 1)
    got = e.range_facets([RangeRequest(x, "size", edges) for x in filters])
    assert len(got) == len(filters)
    for x, r in zip(filters, got):
        v = size[members[x]]
        want = ([int(((v >= lo) & (v < hi)).sum()) for lo, hi in zip(edges, edges[1:])], int((v < edges[0]).sum()), int((v >= edges[-1]).sum()), 0, len(v),
                int(v.min()) if len(v) else None, int(v.max()) if len(v) else None)
        assert r.error is None and (r.counts, r.below, r.above, r.nan, r.total, r.min, r.max) == want, (n, x, r, want)

    whole = e.field_stats([StatsRequest(x, "size") for x in filters])
    grouped = e.field_stats([StatsRequest(x, "size", "shade") for x in filters])
    assert len(whole) == len(grouped) == len(filters)
    for x, w, g in zip(filters, whole, grouped):
        d = members[x]
        v = size[d]
        figures = lambda u: (len(u), int(u.min()) if len(u) else None, int(u.max()) if len(u) else None, int(u.sum()))
        for st in (w, g):
            assert st.error is None and (st.count, st.min, st.max, st.sum) == figures(v) and (st.nan, st.total) == (0, len(v)), (n, x, st, figures(v))
        assert w.groups == []
        want = {s: figures(v[[shade[i] == s for i in d]]) for s in set(shade[i] for i in d)}
        assert {grp.value: (grp.count, grp.min, grp.max, grp.sum) for grp in g.groups} == want and len(g.groups) == len(want), (n, x, g.groups, want)
        assert all(grp.nan == 0 for grp in g.groups)
