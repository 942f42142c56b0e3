"""field_distinct on the GPU: the exact number of distinct values of a field over the documents a filter accepts, whole and per group.

Expected numbers come from numpy on the columns' VALUES, on the corpus of test_gpu_field_stats.py (4 099 documents: 256 walk groups of 16 and a partial last
one, three of them deleted) with test_gpu_top_groups.py's unique column: len(np.unique(...)) of the members' values, whole and per group, sizes by counting.
A double is told apart by its bit pattern (the dictionary's rule: -0.0 and 0.0 are two values, the NaNs here share one payload), and the whole count of the
double column is ALSO held to list_groups(...).total_groups, which is the definition.  Fields of 1 (one), 7 (tag), 3000 (g3000) and 4 099 (uniq) values and
the double column price; group_by None, one, tag, g3000 and the field itself.

Every case runs in automatic placement and forced into LDS, the global bitmap and the hash set, and all four answer with the same repr.  At 4 099 documents
the hash set has 16 384 slots (the power of two >= 2 x 4 099 pairs): 4 099 members into 7 pairs have many threads install the same key or bit, 4 099
members into 4 099 pairs collide and chain at a quarter load.  Nothing here tries to raise the overflow flag: that path is the host model's
(tests/test_distinct_model.py)."""
import numpy as np
import pytest

from infidex_amd import DistinctRequest, Document, SearchEngine
from infidex_amd.engine import Session
from tests.test_gpu_field_stats import D, FILTERS
from tests.test_gpu_top_groups import TopModel, build

pytestmark = pytest.mark.gpu

FIELDS = ["one", "tag", "g3000", "uniq", "price"]
GROUPS = [None, "one", "tag", "g3000"]
SETS = FILTERS + ["num < 20"]                  # every live document, selective ones, one that accepts nothing ("num = 1000"), the last document alone
AUTO, LDS, BITMAP, HASH = 0, 1, 2, 3


def values(m, name):
    """the column as what tells its values apart: a double by its bits"""
    col = getattr(m, name)
    return col.view(np.uint64) if col.dtype.kind == "f" else col


class Expect:
    def __init__(self, m):
        self.m = m; self.cache = {}

    def __call__(self, r):
        """(distinct, total, [(value, size, distinct)]) of a DistinctRequest"""
        m = self.m
        key = (r.filter, r.field, r.group_by, m.live.tobytes())
        if key not in self.cache:
            live = m.members(r.filter); f = values(m, r.field)
            groups = []
            if r.group_by is not None:
                g = getattr(m, r.group_by); ids = np.nonzero(live)[0]
                order = ids[np.argsort(g[ids], kind="stable")]
                cuts = np.nonzero(g[order][1:] != g[order][:-1])[0] + 1
                for part in np.split(order, cuts) if len(order) else []:
                    groups.append((str(g[part[0]]), len(part), len(np.unique(f[part]))))
                groups.sort(key=lambda t: (-t[1], t[0]))          # members descending, then the value's text ascending (ASCII here): field_stats' order
            self.cache[key] = (len(np.unique(f[live])), int(live.sum()), groups)
        return self.cache[key]


def check(want, got, r):
    """one answered request against the model, and the invariants of every answer"""
    distinct, total, groups = want(r)
    assert got.error is None, (r, got.error)
    assert (got.distinct, got.total) == (distinct, total), (r, got.distinct, got.total, distinct, total)
    assert [(g.value, g.size, g.distinct) for g in got.groups] == groups, (r, got.groups[:3], groups[:3])
    if r.group_by is None:
        assert got.groups == []
    else:
        assert sum(g.size for g in got.groups) == got.total
        assert max([g.distinct for g in got.groups], default=0) <= got.distinct <= sum(g.distinct for g in got.groups)
        assert all(1 <= g.distinct <= g.size for g in got.groups)


def run(e, want, reqs):
    got = e.field_distinct(reqs)
    assert len(got) == len(reqs)
    for g, r in zip(got, reqs):
        check(want, g, r)
    return got


@pytest.fixture(scope="module")
def fx():
    m = TopModel()
    return build(m), m, Expect(m)


def test_the_columns_are_what_the_cases_need():
    m = TopModel()
    assert [len(np.unique(values(m, f))) for f in FIELDS[:4]] == [1, 7, 3000, D]
    price = m.price[m.live]
    assert np.isnan(price).any() and (np.signbit(price) & (price == 0)).any() and (~np.signbit(price) & (price == 0)).any()
    assert len(np.unique(values(m, "price")[m.live])) == len(np.unique(price[~np.isnan(price)])) + 2       # one NaN payload; -0.0 apart from 0.0
    assert m.members("num = 1000").sum() == 0 and m.members("idx = %d" % (D - 1)).sum() == 1 and 0 < m.members("num = 3").sum() < 100


@pytest.mark.parametrize("field", FIELDS)
def test_every_case_in_every_placement_is_the_model_and_the_same_bytes(fx, field):
    e, m, want = fx
    s = Session(e)
    try:
        groups = GROUPS + ([field] if field not in GROUPS + ["uniq", "price"] else [])
        reqs = [DistinctRequest(x, field, g) for g in groups for x in SETS]
        seen = {}
        for mode in (AUTO, LDS, BITMAP, HASH):
            s.set_distinct_placement(mode)
            got = []
            for r0 in range(0, len(reqs), 16):
                got += run(s, want, reqs[r0:r0 + 16])
                lds, bitmap, hashed = s.last_field_distinct_stats()[2:5]
                if mode == HASH:
                    assert (lds, bitmap) == (0, 0) and hashed > 0
                if mode == BITMAP:
                    assert lds == 0 and bitmap > 0
            seen[mode] = [repr(a) for a in got]
        assert seen[AUTO] == seen[LDS] == seen[BITMAP] == seen[HASH]
        # the whole count is list_groups' number of groups of the field, and the sizes are field_stats' member counts
        s.set_distinct_placement(AUTO)
        for x in SETS:
            whole = s.field_distinct(x, field)
            assert whole.distinct == s.list_groups(x, field).total_groups and whole.total == s.list_documents(x).total, (x, field)
            for g in ("tag", "g3000"):
                st = s.field_stats(x, "qty", g)
                got = s.field_distinct(x, field, g)
                assert [(a.value, a.size) for a in got.groups] == [(b.value, b.count + b.nan) for b in st.groups] and got.total == st.total
    finally:
        s.close()


def test_a_group_by_the_field_itself_has_one_value_per_group(fx):
    e, m, want = fx
    for f in ("one", "tag", "g3000"):
        for x in SETS:
            got = run(e, want, [DistinctRequest(x, f, f)])[0]
            assert all(g.distinct == 1 for g in got.groups) and len(got.groups) == got.distinct


def test_placements_chosen_forced_and_fallen_back(fx):
    e, m, want = fx
    s = Session(e)
    try:
        def place(mode, field, g):
            s.set_distinct_placement(mode)
            run(s, want, [DistinctRequest(None, field, g)])
            return s.last_field_distinct_stats()[2:5]
        # rows x words per row + size counters: 1 x 129 + 1 and 7 x 129 + 7 words fit a workgroup's LDS; 3000 x 129 words do not fit a CU's
        assert place(AUTO, "uniq", None) == (1, 0, 0) and place(AUTO, "uniq", "tag") == (1, 0, 0) and place(AUTO, "tag", "g3000") == (1, 0, 0)
        # 3000 rows of 129 words (1.5 MB) against a hash set of 16 384 slots (128 KiB): the smaller workspace
        assert place(AUTO, "uniq", "g3000") == (0, 0, 1)
        assert place(LDS, "uniq", "g3000") == (0, 1, 0)           # forced into LDS, it does not fit: the next larger placement
        assert place(BITMAP, "uniq", "g3000") == (0, 1, 0) and place(HASH, "uniq", "g3000") == (0, 0, 1)
        assert place(BITMAP, "one", None) == (0, 1, 0) and place(HASH, "one", None) == (0, 0, 1) and place(LDS, "one", None) == (1, 0, 0)
        # launches: the walk, the count of the rows and — more than one row — their union and its count; the hash set counts as it installs
        s.set_distinct_placement(AUTO)
        run(s, want, [DistinctRequest(None, "tag", None)]); assert s.last_field_distinct_stats() == (0, 0, 1, 0, 0, 2)
        run(s, want, [DistinctRequest(None, "tag", "one")]); assert s.last_field_distinct_stats() == (0, 0, 1, 0, 0, 2)      # (one group value: one row)
        run(s, want, [DistinctRequest(None, "uniq", "tag")]); assert s.last_field_distinct_stats() == (0, 0, 1, 0, 0, 4)
        s.set_distinct_placement(HASH)
        run(s, want, [DistinctRequest(None, "uniq", None)]); assert s.last_field_distinct_stats() == (0, 0, 0, 0, 1, 1)
        run(s, want, [DistinctRequest(None, "uniq", "tag")]); assert s.last_field_distinct_stats() == (0, 0, 0, 0, 1, 2)     # (the side row's count)
    finally:
        s.close()


@pytest.mark.parametrize("mode", [LDS, BITMAP, HASH])
def test_two_race_shapes(fx, mode):
    """4 099 members into 7 pairs: many threads set the same bit or install the same key, each counted once.  4 099 members into 4 099 pairs: in the hash set
    collisions and probe chains.  The same by 7 groups: 7 and 4 099 pairs again, now over 7 rows."""
    e, m, want = fx
    s = Session(e)
    try:
        s.set_distinct_placement(mode)
        reqs = [DistinctRequest(None, "tag", None), DistinctRequest(None, "uniq", None), DistinctRequest(None, "tag", "tag"), DistinctRequest(None, "uniq", "tag"),
                DistinctRequest("num >= 0", "tag", None), DistinctRequest("num >= 0", "uniq", "one")]
        first = run(s, want, reqs)
        assert (first[0].distinct, first[1].distinct, first[0].total) == (7, D - 3, D - 3)
        for _ in range(3):
            assert run(s, want, reqs) == first
    finally:
        s.close()


def test_the_same_bytes_alone_among_sixteen_with_refusals_and_on_two_sessions(fx):
    e, m, want = fx
    s, t = Session(e), Session(e)
    try:
        bad = [DistinctRequest("num = ", "tag"), DistinctRequest(None, "nosuch"), DistinctRequest("tag MATCHES 't[12]'", "tag", "one")]
        others = [DistinctRequest(["num < 20", None, "tag = 't1'"][i % 3], FIELDS[i % 5], GROUPS[i % 4]) for i in range(12)]
        for probe in (DistinctRequest("num < 20", "uniq", "g3000"), DistinctRequest(None, "price", "tag"), DistinctRequest("num = 3", "g3000", None)):
            for mode in (AUTO, LDS, BITMAP, HASH):
                s.set_distinct_placement(mode); t.set_distinct_placement(mode)
                alone = s.field_distinct([probe])[0]
                check(want, alone, probe)
                for at in (1, 7, 12):                             # refused requests first, in the middle and last
                    call = [bad[0]] + others[:6] + [bad[1]] + others[6:] + [bad[2]]
                    call.insert(at, probe)
                    assert len(call) == 16
                    among = s.field_distinct(call)
                    assert repr(among[at]) == repr(alone)
                    assert [a.error is not None for a in among] == [r in bad for r in call]
                    for a, r in zip(among, call):
                        if a.error is None:
                            check(want, a, r)
                assert repr(t.field_distinct([probe])[0]) == repr(alone)
                assert repr(t.field_distinct(others)) == repr(s.field_distinct(others))
    finally:
        s.close(); t.close()


def test_refusals_are_per_request_with_field_stats_messages(fx):
    e, m, want = fx
    bad = [(DistinctRequest("num = ", "tag"), "syntax"), (DistinctRequest("tag MATCHES 't[12]'", "tag"), "MATCHES"), (DistinctRequest(None, None), "needs a field"),
           (DistinctRequest(None, "nosuch"), "no field named 'nosuch'"), (DistinctRequest(None, "tag", "nosuch"), "no group_by field named 'nosuch'"),
           (DistinctRequest(None, "tag", "uniq"), "has more than 4096 distinct values"), (DistinctRequest(None, "uniq", "uniq"), "has more than 4096 distinct values")]
    for b, word in bad:
        a = e.field_distinct([b])[0]
        assert a.error and word.lower() in a.error.lower() and a.groups == [] and a.total == a.distinct == 0, (b, a.error)
    # the group_by messages are field_stats' own, under this call's name
    for g in ("nosuch", "uniq"):
        assert e.field_distinct(None, "tag", g).error == e.field_stats(None, "qty", g).error.replace("field_stats", "field_distinct")
    assert e.field_distinct("num = ", "tag").error == e.field_distinct([bad[0][0]])[0].error


def test_passes_and_masks_are_shared(fx):
    e, m, want = fx
    s = Session(e)
    try:
        x = "num < 20 AND idx >= 0"                                 # (a filter no other test has built a mask of on this session)
        run(s, want, [DistinctRequest(x, "uniq", "tag")] * 16)
        assert s.last_field_distinct_stats() == (1, 0, 1, 0, 0, 1 + 4)      # sixteen requests of one spec: ONE walk; the mask build, the walk, count, union, count
        run(s, want, [DistinctRequest(x, "uniq", "tag"), DistinctRequest(x, "uniq", None), DistinctRequest(x, "tag", "tag"), DistinctRequest(x, "uniq", "tag")])
        assert s.last_field_distinct_stats()[:5] == (0, 1, 3, 0, 0)         # another group column and another field are specs of their own
        run(s, want, [DistinctRequest(None, "tag")])
        assert s.last_field_distinct_stats()[:2] == (0, 0)                  # the index's Deleted flags, no mask
        seventeen = [DistinctRequest("num = %d" % i, "uniq", "tag") for i in range(17)]      # Python splits: 16 + 1
        got = run(s, want, seventeen)
        assert len(got) == 17 and s.last_field_distinct_stats()[:3] == (1, 0, 1)
        assert s.list_documents("num = 16").total == got[16].total and s.last_list_stats()[:2] == (0, 1)      # the mask serves list_documents
    finally:
        s.close()


@pytest.mark.parametrize("n", list(range(1, 49)))
def test_small_corpora_every_shape_of_the_partial_last_group(n):
    """Corpora of up to three groups of 16: the flags of the partial last group are read one by one.  The filters leave runs of accepted and refused
    documents that begin and end at every position of a group of four."""
    words = ["alpha", "bravo", "charlie", "delta", "echo", "foxtrot", "golf", "hotel"]
    shade = np.array((["red", "blue", "green"] * 16)[:n])
    size = np.arange(1, n + 1, dtype=np.int64)
    half = np.array([0.0, -0.0, np.nan, 1.5, 1.5] * 10)[:n]
    e = SearchEngine.create_default(device=0)
    e.index_documents([Document(100 + i, "%s %s item %d" % (words[i % 8], words[(i * 3 + 1) % 8], i)) for i in range(n)])
    e.set_column("shade", list(shade), facetable=True); e.set_column("size", size, facetable=False); e.set_column("half", half, facetable=False)
    filters = ["size >= %d" % v for v in range(1, n + 2)] + ["size <= %d" % v for v in range(1, n)] + ["size = 5", "size = 6 OR size = 11", "size = 9 OR size >= 13", None]
    cols = {"shade": shade, "size": size, "half": half.view(np.uint64)}
    reqs = [DistinctRequest(x, f, g) for x in filters for f, g in (("size", None), ("shade", None), ("half", "shade"), ("size", "shade"), ("shade", "shade"))]
    seen = []
    for mode in (AUTO, LDS, BITMAP, HASH):
        e.set_distinct_placement(mode)
        got = []
        for r0 in range(0, len(reqs), 16):
            got += e.field_distinct(reqs[r0:r0 + 16])
        for a, r in zip(got, reqs):
            live = np.array([_accepts(r.filter, int(v)) for v in size])
            f = cols[r.field]
            groups = []
            if r.group_by:
                groups = [(str(gv), int((live & (shade == gv)).sum()), len(np.unique(f[live & (shade == gv)]))) for gv in np.unique(shade[live])]
                groups.sort(key=lambda t: (-t[1], t[0]))
            assert a.error is None and (a.distinct, a.total) == (len(np.unique(f[live])), int(live.sum())), (n, mode, r, a)
            assert [(g.value, g.size, g.distinct) for g in a.groups] == groups, (n, mode, r, a.groups, groups)
        seen.append([repr(a) for a in got])
    assert seen[0] == seen[1] == seen[2] == seen[3]


def _accepts(x, v):
    """the small corpora's filters on a value of `size`"""
    if x is None:
        return True
    return bool(eval(x.replace("size", str(v)).replace(" = ", " == ").replace("OR", "or")))


def test_deletions_and_a_restore_follow_the_model(fx):
    e, m, want = fx
    s = Session(e)
    try:
        reqs = [DistinctRequest(None, "uniq", "tag"), DistinctRequest("num < 20", "g3000", "tag"), DistinctRequest(None, "price", None),
                DistinctRequest("idx = %d" % (D - 1), "uniq", "one")]
        before = run(s, want, reqs)
        assert s.field_distinct(reqs) == before and s.last_field_distinct_stats()[:2] == (0, 2)
        gone = sorted({D - 1} | set(range(3, D, 11)))
        try:
            assert e.delete_documents(m.keys[gone]) == len([d for d in gone if m.live[d]])
            m.live = m.live0.copy(); m.live[gone] = False
            got = run(s, want, reqs)
            assert s.last_field_distinct_stats()[:2] == (2, 0)      # the epoch moved: every mask is built again
            lost = len([d for d in gone if m.live0[d]])
            assert got[0].total == before[0].total - lost and got[0].distinct == before[0].distinct - lost
            assert (got[3].distinct, got[3].total, got[3].groups) == (0, 0, [])
        finally:
            e.restore_documents(); m.live = np.ones(D, bool)
        after = run(s, want, reqs)                                  # everything lives: the three documents deleted at the start too
        assert after[0].total == D == after[0].distinct
        assert e.delete_documents(m.keys[~m.live0]) == 3
        m.live = m.live0.copy()
        assert run(s, want, reqs) == before
    finally:
        m.live = m.live0.copy()
        s.close()
