"""list_group_members through the frame of the engine's per-request calls (set_call, infidex_amd/csrc/host/engine.cpp) on the GPU:
tests/test_gpu_set_call_frame.py's check for the eighth feature the frame carries.

The corpus is that file's, rebuilt here: 37 documents (two whole groups of sixteen and a partial one, four of them deleted) with an int64 column, a double
column with a NaN, a string column and two group columns.  ONE call of sixteen requests: refused ones at the first, a middle and the last position (an
unknown field, a filter with a syntax error, a per_group of 0) between answered ones that repeat filters and interleave masks, order columns, group columns
and per_group, so that the device call orders them differently from the caller.  Every answered request equals the same request asked alone in a call of
its own, every refused one carries the message it gets alone, and the masks the call built plus the ones it reused are the distinct filters that compile.
Every comparison is exact equality."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, GroupMembersRequest
from infidex_amd.engine import Session

pytestmark = pytest.mark.gpu

N = 37
A, B, C3 = "size >= 10", "shade = 'red'", "size < 30 AND shape != 'disc'"      # the filters that compile; None: every live document
BAD = "size = "                                                                # a syntax error


@pytest.fixture(scope="module")
def engine():
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    size = (np.arange(N, dtype=np.int64) * 7) % 41 - 5
    price = ((np.arange(N) * 13) % 17).astype(np.float64) / 4 - 1.5; price[5] = np.nan
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(N)])
    e.set_column("size", size, facetable=False); e.set_column("price", price, facetable=False)
    e.set_column("name", ["n%02d" % ((i * 5) % 23) for i in range(N)], facetable=False)
    e.set_column("shade", (["red", "blue", "green"] * 13)[:N], facetable=True)
    e.set_column("shape", (["disc", "cube", "cone", "ring", "disc"] * 8)[:N], facetable=True)
    assert e.delete_documents([102, 116, 117, 136]) == 4
    return e


@pytest.fixture
def sessions(engine):
    both = [Session(engine), Session(engine)]      # fresh mask caches: one for the call of sixteen, one for the requests asked alone
    yield both
    for s in both:
        s.close()


def test_sixteen_requests_in_one_call_equal_each_asked_alone(engine, sessions):
    M = GroupMembersRequest
    reqs = [M(A, "nosuch", "size"), M(A, "shade", "size", True, 3, 0, 5), M(B, "shape", "price", False, 2, 1, 40), M(None, "shape", None, True, 16, 0, 10),
            M(A, "shape", "size", True, 1, 0, 40), M(C3, "shade", "name", False, 16, 0, 40), M(B, "shade", "size", True, 2, 0, 40), M(BAD, "shade", "size"),
            M(C3, "shape", "size", False, 3, 1, 3), M(A, "shade", "price", False, 4, 0, 5), M(None, "name", "shade", False, 2, 0, 40), M(B, "shape", "price", False, 16, 0, 1),
            M(A, "shade", "size", True, 5, 1, 2), M(C3, "size", None, True, 3, 2, 40), M(A, "shape", "name", True, 7, 0, 40), M(B, "shade", "size", True, 0)]
    refused, filters = {0: "nosuch", 7: "syntax", 15: "per_group"}, 3
    ask = lambda r, k: sessions[k].list_group_members(r)
    together, alone = ask(reqs, 0), [ask([r], 1)[0] for r in reqs]
    built, reused = sessions[0].last_group_members_stats()[:2]
    assert len(reqs) == 16 and len(together) == 16
    for i, (t, a) in enumerate(zip(together, alone)):
        assert repr(t) == repr(a), (i, reqs[i], t, a)
        assert (t.error is not None) == (i in refused) and (i not in refused or refused[i] in t.error), (i, reqs[i], t)
    assert built + reused == filters and built == filters, (built, reused)
    again = ask(reqs, 0)
    assert [repr(t) for t in again] == [repr(t) for t in together] and sessions[0].last_group_members_stats()[:2] == (0, filters)
    # the answered ones are not empty, and the members of a row are members of its group in the listing's order: request 1 against list_documents
    assert all(t.groups and all(g.document_ids and len(g.document_ids) == min(g.size, r.per_group) for g in t.groups) for i, (t, r) in enumerate(zip(together, reqs)) if i not in refused)
    for g in together[1].groups:
        w = engine.list_documents("(%s) AND shade = '%s'" % (A, g.group_value), "size", True, 0, 3)
        assert (g.document_ids, g.values, g.size) == (w.document_ids, w.values, w.total)
