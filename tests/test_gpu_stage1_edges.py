"""Stage 1 held to tests/stage1_model.py on constructed postings, through the raw C ABI (include/infidex_hip.h), at EVERY range width infx_create accepts —
512, 1024, 2048, 4096, 8192 and 16384 documents per LDS range block, each a template instantiation of k_accumulate / k_accumulate_sparse / k_union and a
different skip-table and replay geometry — and under three splits between the two accumulation kernels (INFX_ACC_SPARSE_T unset: the default split; 0: the
streaming kernel alone; 4096: nearly everything to the sparse kernel, in many rounds).  No text, no oracle: the index is stage1_model.EdgeIndex, whose lists
put postings on and beside every range and stripe boundary, hold 63 and 64 postings (the skip-table threshold), leave whole ranges empty, and carry every tf
byte from 1 to 255; the queries are stage1_model.edge_batch.  The variable is read once per process, so every case is one child process; children run one
after the other, each under its own time limit, and once one ends abnormally (a signal, an abort, its time limit) no further child is started.

Held, for every query, with the exact replay off (INFX_CFG_NO_EXACT_REPLAY) and on, before and after infx_set_deleted on {kR} and N - 1, in batches of one,
two and four mask words:
  - infx_stage1_accumulate's 136 class counts equal the model's exactly;
  - infx_stage1_select's hit count is the model's; every returned document is a model row whose score is within (10 + n_terms) * 2^-24 of the float64 model
    (stage1_model.tolerance: nine roundings per term — infidex_hip.hip k_doc_norm's three and the 0.75f / avgdl in front of it, stage1.hip.inc:305-307's
    five — and one per accumulation, :308);
  - the returned set is the model's top `depth` except among documents whose model score lies within that tolerance of the cut, at most 2 % of the rows;
    a query with no more rows than `depth` matches row for row;
  - the three forms of a virtual term (device union, member list, caller's union) return identical rows;
  - the rows and counts of one width are byte-identical across the three split settings.

The mode of a query is the batch's own — the ABI takes it from the host — and roles, ranks, n_and, df_s1 and df_s2 are the model's reading of the rules for
that mode and the idf handed over.  By those rules the half-full list t6 and the full list t7 are low-quality terms beside a rare one: in queries 5, 6, 10 and
12 they still set candidate bits and score (several rounds per range at every R), and it is the class counts that make infx_stage1_select drop their rows.
Queries 15 and 16 (t6 alone, t7 alone) and the prefix query over range 1 are where a cut runs through thousands of rows.  The DocSet of range 1 holds every
(R / 4096)-th document from R = 8192 on, so that it stays within the 10 * depth documents prefix precedence accepts.
This index gives every document its own length, so no tie is structural and a query is rarely if ever flagged: the exact replay is not exercised here.  That is
done by tests/test_gpu_replay_plateaus.py (the replay kernels against tests/replay_model.py on constructed score plateaus, bit for bit).
First run on an MI355X: every case passed with no row excused at any cut."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stage1_model as M

pytestmark = pytest.mark.gpu
SPLITS = (None, "0", "4096")
CHILD_TIMEOUT = 180

CHILD = r'''
import ctypes as C, sys
import numpy as np
from infidex_amd.engine import load_library, _p
from tests.test_gpu_device_abi import Cfg, Term, Query, Hit, chk
from tests import stage1_model as M
R, out = int(sys.argv[1]), sys.argv[2]
L = load_library()
E = M.EdgeIndex(R); N, DEPTH = E.N, M.EDGE_DEPTH
f32 = np.float32
res = {}
for flags in (1, 0):                                     # INFX_CFG_NO_EXACT_REPLAY, then with the replay behind the first pass
    idx = C.c_void_p(); st = C.c_void_p()
    cfg = Cfg(0, R, DEPTH, flags)
    chk(L, L.infx_create(C.byref(cfg), C.byref(idx)))
    keys = np.arange(N, dtype=np.int64)
    chk(L, L.infx_upload_docs(idx, N, _p(E.doc_len, C.c_float), C.c_float(E.avgdl), _p(keys, C.c_int64), None, None, None))
    chk(L, L.infx_upload_postings(idx, E.T, _p(E.post_off, C.c_uint64), _p(E.post_doc, C.c_int32), _p(E.post_w, C.c_uint8), _p(E.df, C.c_int32)))
    soff = np.zeros(len(E.sets) + 1, np.uint64); soff[1:] = np.cumsum([len(s) for s in E.sets]); sdocs = np.concatenate(E.sets).astype(np.int32)
    chk(L, L.infx_upload_prefix_docsets(idx, len(E.sets), _p(soff, C.c_uint64), _p(sdocs, C.c_int32)))
    chk(L, L.infx_stream_create(idx, C.byref(st)))
    moffs = np.asarray([0, len(M.UNION_MEMBERS)], np.uint32); mem = np.asarray(M.UNION_MEMBERS, np.int32); ucnt = np.zeros(1, np.uint32)
    for deleted in (0, 1):
        if deleted:
            flagsN = np.zeros(N, np.uint8); flagsN[E.gone] = 1
            chk(L, L.infx_set_deleted(idx, N, _p(flagsN, C.c_uint8)))
        for level in (0, 1, 2):
            qs, terms, extra = [], [], []
            for Q in M.edge_batch(E, level):
                mt, P, _, _, _ = M.edge_model(E, Q)
                ids = ([-1] if Q["virt"] is not None else []) + Q["terms"]
                qs.append(Query(len(terms), len(ids), P.mode, Q["pset"], DEPTH, P.n_and, P.df_s1, P.df_s2))
                for t, tid, role, rank in zip(mt, ids, P.roles, P.ranks):
                    idf = float(t.idf); mx = float(f32(t.idf * f32(3.2)))
                    if tid >= 0: terms.append(Term(tid, 0, 0, idf, mx, role, rank, 0))
                    elif Q["virt"] == 2: terms.append(Term(-1, 0, 0, idf, mx, role, rank, 2))                                   # union 0 of the last infx_union_build
                    elif Q["virt"] == 1: terms.append(Term(-1, len(extra), len(mem), idf, mx, role, rank, 1)); extra += mem.tolist()
                    else: terms.append(Term(-1, len(extra), len(t.docs), idf, mx, role, rank, 0)); extra += t.docs.tolist()
            nq = len(qs)
            QA = (Query * nq)(*qs); TA = (Term * len(terms))(*terms); EX = np.asarray(extra, np.int32)
            chk(L, L.infx_union_build(st, 1, _p(moffs, C.c_uint32), _p(mem, C.c_int32), _p(ucnt, C.c_uint32)))
            counts = np.zeros((nq, M.NCLASS), np.uint32)
            chk(L, L.infx_stage1_accumulate(st, nq, QA, len(terms), TA, len(EX), _p(EX, C.c_int32), counts.ctypes.data_as(C.c_void_p)))
            hits = (Hit * (nq * DEPTH))(); hc = np.zeros(nq, np.uint32)
            chk(L, L.infx_stage1_select(st, nq, counts.ctypes.data_as(C.c_void_p), hits, _p(hc, C.c_uint32)))
            h = np.frombuffer(hits, dtype=[("doc", np.int32), ("score", np.uint32)]).reshape(nq, DEPTH).copy()
            for i in range(nq): h[i, int(hc[i]):] = 0
            tag = "f%d_d%d_l%d_" % (flags, deleted, level)
            res[tag + "counts"] = counts; res[tag + "hc"] = hc; res[tag + "doc"] = h["doc"]; res[tag + "score"] = h["score"]; res[tag + "union"] = ucnt.copy()
    L.infx_stream_destroy(st); L.infx_destroy(idx)
np.savez(out, **res)
'''

_stop = []          # why nothing more is started on the GPU
_runs = {}
_model = {}


def run_child(R, split, tmp):
    key = (R, split)
    if key in _runs:
        return _runs[key]
    if _stop:
        pytest.fail("no further child is started: " + _stop[0])
    env = dict(os.environ); env.pop("INFX_ACC_SPARSE_T", None)
    if split is not None:
        env["INFX_ACC_SPARSE_T"] = split
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp / f"edges_{R}_{split}.npz")
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, str(R), out], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _stop.append(f"the child of R = {R}, INFX_ACC_SPARSE_T = {split} ran into its time limit")
        pytest.fail(_stop[0])
    if p.returncode != 0:
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            _stop.append(f"the child of R = {R}, INFX_ACC_SPARSE_T = {split} ended abnormally ({p.returncode})")
        pytest.fail(f"child R = {R}, INFX_ACC_SPARSE_T = {split}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    _runs[key] = dict(np.load(out))
    return _runs[key]


def model_of(R):
    """Per deletion state and query of the widest batch: (name, n_terms, counts, rows, top)."""
    if R not in _model:
        E = M.EdgeIndex(R)
        _model[R] = []
        for deleted in (False, True):
            per = []
            for Q in M.edge_batch(E, 2):
                terms, P, sc, counts, rw = M.edge_model(E, Q, deleted)
                per.append((Q["name"], len(terms), counts, rw, M.top(rw, M.EDGE_DEPTH)))
            _model[R].append(per)
    return _model[R]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("stage1_edges")


@pytest.mark.parametrize("split", SPLITS, ids=["default", "stream", "sparse"])
@pytest.mark.parametrize("R", M.WIDTHS)
def test_constructed_postings_against_the_model(R, split, tmp):
    res = run_child(R, split, tmp)
    model = model_of(R)
    E = M.EdgeIndex(R)
    excused = worst = 0
    for flags in (1, 0):
        for deleted in (0, 1):
            for level in (0, 1, 2):
                tag = f"f{flags}_d{deleted}_l{level}_"
                names = [Q["name"] for Q in M.edge_batch(E, level)]
                assert [m[0] for m in model[deleted]][:len(names)] == names
                assert int(res[tag + "union"][0]) == len(np.unique(np.concatenate([E.lists[t] for t in M.UNION_MEMBERS])))
                got_rows = {}
                for i, (name, nt, counts, rw, want) in enumerate(model[deleted][:len(names)]):
                    what = (R, split, tag, name)
                    c = res[tag + "counts"][i]
                    assert np.array_equal(c, counts), (what, "counts", {j: (int(c[j]), int(counts[j])) for j in range(M.NCLASS) if c[j] != counts[j]})
                    n = int(res[tag + "hc"][i])
                    docs = res[tag + "doc"][i, :n].tolist(); sc = res[tag + "score"][i, :n].view(np.float32).tolist()
                    assert len(set(docs)) == n, (what, "a document twice")
                    got = dict(zip(docs, sc))
                    x = M.check_rows(got, rw, M.EDGE_DEPTH, nt, what, want=want)
                    excused += x; worst = max(worst, x / max(n, 1))
                    got_rows[name] = got
                assert got_rows["12 union built"] == got_rows["12 union members"] == got_rows["12 union caller"], (R, split, tag)
    print(f"R = {R}, INFX_ACC_SPARSE_T = {split}: {excused} rows excused at a cut over all batches, at most {100 * worst:.2f} % of one query's")
    if split is not None:                                 # the same bytes whichever kernel took a (query, stripe) pair
        base = run_child(R, None, tmp)
        assert sorted(base) == sorted(res)
        for k in base:
            assert np.array_equal(base[k], res[k]), (R, split, k)
