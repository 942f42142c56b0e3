"""The frame of the engine's per-request calls (set_call, infidex_amd/csrc/host/engine.cpp) on the GPU for the ninth kind it carries, bucket_stats: the check of
tests/test_gpu_set_call_frame.py on that file's corpus, restated here.

37 documents (two whole groups of sixteen and a partial one, four of them deleted) with an int64 column, a double column with a NaN, a string column and two
group columns.  ONE call of sixteen requests: refused ones at the first, a middle and the last position (an unknown field, a filter with a syntax error, a
string bucket_by, edges that do not increase) between answered ones that repeat filters and interleave masks, value columns and bucket columns, so that the
device call orders them differently from the caller.  Every answered request equals the same request asked alone in a call of its own, every refused one
carries the message it gets alone, and the masks the call built plus the ones it reused are the distinct filters that compile.  Every comparison is exact
equality."""
import numpy as np
import pytest

from infidex_amd import SearchEngine, Document, BucketStatsRequest
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


def held(ask, stats, reqs, refused, filters):
    """ask(reqs) in one call on a session of its own against ask([r]) per request on another; refused: place -> a word of its message."""
    together, alone = ask(reqs, 0), [ask([r], 1)[0] for r in reqs]
    built, reused = stats(0)[:2]
    assert len(reqs) == 16 and set(refused) >= {0, 15} and len(together) == 16
    for i, (t, a) in enumerate(zip(together, alone)):
        assert repr(t) == repr(a), (i, reqs[i], t, a)
        assert (t.error is not None) == (i in refused) and (i not in refused or refused[i] in t.error), (i, reqs[i], t)
    assert built + reused == filters and built == filters, (built, reused)
    again = ask(reqs, 0)
    assert [repr(t) for t in again] == [repr(t) for t in together] and stats(0)[:2] == (0, filters)


@pytest.fixture
def sessions(engine):
    both = [Session(engine), Session(engine)]      # fresh mask caches: one for the call of sixteen, one for the requests asked alone
    yield both
    for s in both:
        s.close()


def test_bucket_stats(engine, sessions):
    R, ei, ed = BucketStatsRequest, (-5, 0, 10, 36), (-1.5, 0.0, 1.25, 3.0)
    reqs = [R(A, "nosuch", "size", ei), R(A, "size", "size", ei), R(B, "price", "price", ed), R(None, "size", "price", (0.0, 1.0)), R(A, "price", "size", ei),
            R(C3, "size", "price", ed), R(B, "size", "size", (-100, 100)), R(BAD, "size", "size", ei), R(C3, "price", "price", ed), R(A, "size", "size", tuple(range(-5, 37))),
            R(None, "price", "size", (-10, 10)), R(B, "price", "size", ei), R(A, "size", "name", ei), R(C3, "size", "size", (3, 4)), R(A, "price", "price", (0.0, 0.25)),
            R(B, "size", "size", (5, 5))]
    held(lambda r, k: sessions[k].bucket_stats(r), lambda k: sessions[k].last_bucket_stats_stats(), reqs, {0: "nosuch", 7: "syntax", 12: "string", 15: "increasing"}, 3)
    got = sessions[0].bucket_stats(reqs)
    assert all(x.error or (x.nan.size + x.below.size + sum(b.size for b in x.buckets) + x.above.size == x.total == x.whole.size) for x in got)
    assert got[2].nan.size == 0 and got[3].total == N - 4 and got[3].nan.size == 1 and got[3].nan.nan == 0 and got[8].whole.nan + got[8].whole.count == got[8].total
