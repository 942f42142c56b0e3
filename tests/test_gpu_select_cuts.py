"""The Stage-1 cut (k_rules, k_select_order, k_selg_hist / k_selg_cut / k_selg_gather, k_select) held to tests/select_model.py through the raw C ABI
(include/infidex_hip.h), on the constructed index select_model.SelectIndex: 70 001 documents of chosen fp32 lengths, and named queries each built for ONE path of
k_select — take-all around the sort's capacity and around the depth, fast-path modes 1, 2 and 3, the second attempt, the radix passes through the score and the doc-id
digits, the swept queries (fine, coarse, take-all, refused), the three sources of the best row left out, the flag test on, one ulp below and at the band edge.  No text,
no oracle: tests/test_select_model.py shows on the CPU that every named query lands on its path and that the batch tells four misreadings of the cut from the right one.

One child process per environment setting — unset, INFX_SEL_GIANT_MIN = 64, 20000, 16384 and 0, INFX_SELECT_LPT = 0 — because the variables are read once per process;
children run one after the other, each under its own time limit, and once one ends abnormally (a signal, an abort, its time limit) no further child is started.
(At 20000 the sweeps are not launched on this index: select_giants wants a query whose row bound reaches four times the threshold, 80 000 > 70 001 documents.  16384 is
the setting at which the queries of 40 000 and 70 001 rows are swept and the others of the same batch are not.)

A child runs the batches of 63, 64, 65 and 100 queries (select_model.select_batch: no order kernel at 63, its sort padded to 128 at 65 and 100) and, on a 1000-document
index, 4096 and 4097 one-row queries (at 4097 the order is dropped), each before and after infx_set_deleted on documents inside the plateaus and at the cuts.  For every
batch, after infx_stage1_accumulate, with NOTHING excused and no tolerance:
  1. infx_shard_select with next_out (k_rules on the device, no flags): hit counts, documents and score bits equal the model's cut row for row, IN ORDER; next_out
     equals the model's best row left out bit for bit;
  2. infx_stage1_select on an index created with INFX_CFG_NO_EXACT_REPLAY (the host's make_rule, a null flag pointer): the bytes of 1;
  3. infx_stage1_select with the replay on: infx_last_exact_replays equals the number of queries the model flags, infx_last_replay_stats' why3 the model's counts of
     why 0 and why 1 with why3[2] == 0; a query the model does not flag returns the bytes of 2, a flagged one equals replay_model.replay bit for bit as a set with scores;
  - the class counts equal the model's (the test hands them back to the select);
  - across the children the outputs of 1 to 3 are byte-identical.

Not seen through the ABI: whether the sweep kernels ran (select_model.path_of says when they do).  Confirmed once by hand with a kernel trace of the INFX_SEL_GIANT_MIN=64
child: k_selg_hist, k_selg_cut and k_selg_gather are launched, 18 times each (the three batches of >= 64 queries on the large index, two deletion states, three selects).
First run on an MI355X (33 named queries, 12 batches and 36 selects per child): every child passed with every comparison exact and nothing excused.  Per batch of the
70 001-document index the model flags 15 queries and the replay took exactly those: 5 for an exact plateau (the four plateaus wider than the sort, "band equal"), 10
inside the band; over a child's batches 40 and 80.  Wall time per child, the model's own work in it included: 1.3 - 1.7 s (a child of the edges module does comparable
work); CHILD_TIMEOUT is some twenty times the slowest, a stall guard.  Tried once by hand: with each of select_model.MISREADINGS switched on in the model, the
comparison against the same kernels fails (ties by descending doc id: two rows of equal score swapped in "take-all 499 rows depth 500"; the band compared with >:
"band edge gathered" comes back replayed; next from the cut's bin only: next_out of "take-all depth+1 rows"; rejected rows ignored: 30 hits against 0 in "second
attempt")."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import replay_model as RM
from tests import select_model as SM

pytestmark = pytest.mark.gpu
SETTINGS = ((None, None), ("INFX_SEL_GIANT_MIN", "64"), ("INFX_SEL_GIANT_MIN", "20000"), ("INFX_SEL_GIANT_MIN", "16384"), ("INFX_SEL_GIANT_MIN", "0"), ("INFX_SELECT_LPT", "0"))
IDS = ["unset", "giant-64", "giant-20000", "giant-16384", "giant-0", "lpt-0"]
CHILD_TIMEOUT = 30
BATCHES = [("S", level) for level in range(len(SM.BATCH_SIZES))] + [("T", 4096), ("T", 4097)]

CHILD = r'''
import ctypes as C, json, sys
import numpy as np
from infidex_amd.engine import load_library, _p
from tests.test_gpu_device_abi import Cfg, Term, Query, Hit, chk
from tests import select_model as SM, replay_model as RM, stage1_model as M
from tests.test_gpu_select_cuts import BATCHES, queries_of
out = sys.argv[1]
L = load_library()
res, stats = {}, {}
plans = {}
for which, X in (("S", SM.SelectIndex()), ("T", SM.TinyIndex())):
    N = X.N
    handles = []
    for flags in (1, 0):                                 # INFX_CFG_NO_EXACT_REPLAY, then with the replay behind the first pass
        idx = C.c_void_p(); st = C.c_void_p()
        cfg = Cfg(0, 0, SM.MAX_DEPTH, flags)
        chk(L, L.infx_create(C.byref(cfg), C.byref(idx)))
        keys = np.arange(N, dtype=np.int64)
        chk(L, L.infx_upload_docs(idx, N, _p(X.doc_len, C.c_float), C.c_float(X.avgdl), _p(keys, C.c_int64), None, None, None))
        chk(L, L.infx_upload_postings(idx, X.T, _p(X.post_off, C.c_uint64), _p(X.post_doc, C.c_int32), _p(X.post_w, C.c_uint8), _p(X.df, C.c_int32)))
        if X.sets:
            soff = np.zeros(len(X.sets) + 1, np.uint64); soff[1:] = np.cumsum([len(s) for s in X.sets]); sdocs = np.concatenate(X.sets).astype(np.int32)
            chk(L, L.infx_upload_prefix_docsets(idx, len(X.sets), _p(soff, C.c_uint64), _p(sdocs, C.c_int32)))
        chk(L, L.infx_stream_create(idx, C.byref(st)))
        handles.append((idx, st))
    for deleted in (0, 1):
        if deleted:
            flagsN = np.zeros(N, np.uint8); flagsN[X.gone] = 1
            for idx, _ in handles:
                chk(L, L.infx_set_deleted(idx, N, _p(flagsN, C.c_uint8)))
        for w, arg in BATCHES:
            if w != which:
                continue
            qs, terms = [], []
            for Q in queries_of(w, arg):
                key = (w, tuple(Q["terms"]), Q["depth"], Q["mode"], Q["pset"])
                if key not in plans:
                    plans[key] = X.select(Q)
                S = plans[key]; P = S.plan
                qs.append(Query(len(terms), len(S.terms), P.mode, -1 if Q["pset"] is None else Q["pset"], Q["depth"], P.n_and, P.df_s1, P.df_s2))
                for (name, _), t, role, rank, mx in zip(Q["terms"], S.terms, P.roles, P.ranks, S.max_scores):
                    terms.append(Term(X.id[name], 0, 0, float(t.idf), float(mx), role, rank, 0))
            nq = len(qs); depth = max(q.depth for q in qs)
            QA = (Query * nq)(*qs); TA = (Term * len(terms))(*terms); EX = np.zeros(1, np.int32)
            tag = "%s%d_d%d_" % (w, arg, deleted)
            (ia, sa), (ib, sb) = handles
            def accumulate(st):
                counts = np.zeros((nq, M.NCLASS), np.uint32)
                chk(L, L.infx_stage1_accumulate(st, nq, QA, len(terms), TA, 0, _p(EX, C.c_int32), counts.ctypes.data_as(C.c_void_p)))
                return counts
            def rows(hits, hc):
                h = np.frombuffer(hits, dtype=[("doc", np.int32), ("score", np.uint32)]).reshape(nq, depth).copy()
                for i in range(nq): h[i, int(hc[i]):] = 0
                return h
            # 1. infx_shard_select: k_rules on the device, the best row left out
            counts = accumulate(sa)
            hits = (Hit * (nq * depth))(); hc = np.zeros(nq, np.uint32); nxt = np.zeros(nq, np.float32)
            chk(L, L.infx_shard_select(sa, nq, counts.ctypes.data_as(C.c_void_p), depth, hits, _p(hc, C.c_uint32), _p(nxt, C.c_float)))
            h = rows(hits, hc)
            res[tag + "counts"] = counts; res[tag + "1hc"] = hc; res[tag + "1doc"] = h["doc"]; res[tag + "1score"] = h["score"]; res[tag + "1next"] = nxt.view(np.uint32).copy()
            # 2. infx_stage1_select, the replay off
            counts2 = accumulate(sa)
            hits = (Hit * (nq * depth))(); hc = np.zeros(nq, np.uint32)
            chk(L, L.infx_stage1_select(sa, nq, counts2.ctypes.data_as(C.c_void_p), hits, _p(hc, C.c_uint32)))
            h = rows(hits, hc)
            res[tag + "2counts"] = counts2; res[tag + "2hc"] = hc; res[tag + "2doc"] = h["doc"]; res[tag + "2score"] = h["score"]
            # 3. infx_stage1_select, the replay on
            counts3 = accumulate(sb)
            hits = (Hit * (nq * depth))(); hc = np.zeros(nq, np.uint32)
            chk(L, L.infx_stage1_select(sb, nq, counts3.ctypes.data_as(C.c_void_p), hits, _p(hc, C.c_uint32)))
            h = rows(hits, hc)
            n = C.c_uint32(0); ms = C.c_float(0); why = (C.c_uint32 * 3)()
            chk(L, L.infx_last_exact_replays(sb, C.byref(n))); chk(L, L.infx_last_replay_stats(sb, C.byref(ms), why))
            res[tag + "3counts"] = counts3; res[tag + "3hc"] = hc; res[tag + "3doc"] = h["doc"]; res[tag + "3score"] = h["score"]
            stats[tag] = dict(nq=nq, depth=depth, replays=int(n.value), why=[int(x) for x in why])
    for idx, st in handles:
        L.infx_stream_destroy(st); L.infx_destroy(idx)
np.savez(out, **res)
print("STATS " + json.dumps(stats))
'''


def queries_of(which, arg):
    return SM.select_batch(arg) if which == "S" else SM.tiny_batch(arg)


_stop = []          # why nothing more is started on the GPU
_runs = {}
_model = {}
_index = {}


def run_child(setting, tmp):
    if setting in _runs:
        return _runs[setting]
    if _stop:
        pytest.fail("no further child is started: " + _stop[0])
    env = dict(os.environ)
    for var, _ in SETTINGS[1:]:
        env.pop(var, None)
    if setting[0] is not None:
        env[setting[0]] = setting[1]
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp / f"cuts_{setting[0]}_{setting[1]}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, out], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _stop.append(f"the child of {setting} ran into its time limit")
        pytest.fail(_stop[0])
    if p.returncode != 0:
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            _stop.append(f"the child of {setting} ended abnormally ({p.returncode})")
        pytest.fail(f"child {setting}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    stats = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("STATS "))[6:])
    _runs[setting] = (dict(np.load(out)), stats, time.time() - t0)
    return _runs[setting]


def model_of(which, Q, deleted):
    """(Sel, Cut, replay result or None) of one query, computed once and left unchanged."""
    key = (which, tuple(Q["terms"]), Q["depth"], Q["mode"], Q["pset"], deleted)
    if key not in _model:
        if which not in _index:
            _index[which] = SM.SelectIndex() if which == "S" else SM.TinyIndex()
        S = _index[which].select(Q, bool(deleted))
        C = S.cut()
        R = RM.replay(S.ix, S.terms, S.plan.cand, S.depth, S.max_scores).result if C.flagged else None
        _model[key] = (S, C, R)
    return _model[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("select_cuts")


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_select_against_the_model(setting, tmp):
    res, stats, secs = run_child(setting, tmp)
    flagged_total = [0, 0]
    for which, arg in BATCHES:
        for deleted in (0, 1):
            tag = f"{which}{arg}_d{deleted}_"
            qs = queries_of(which, arg)
            st = stats[tag]
            assert st["nq"] == len(qs)
            why = [0, 0]
            for i, Q in enumerate(qs):
                what = (setting, tag, Q["name"])
                S, Cm, R = model_of(which, Q, deleted)
                for k in ("counts", "2counts", "3counts"):
                    c = res[tag + k][i]
                    assert np.array_equal(c, S.counts), (what, k, {j: (int(c[j]), int(S.counts[j])) for j in range(len(c)) if c[j] != S.counts[j]})
                # 1. the deterministic cut, in order, and the best row left out
                n = int(res[tag + "1hc"][i])
                if which == "S":
                    print(f"{what}: hits {n} / {Cm.hits}, next {int(res[tag + '1next'][i]):#x} / {int(SM.bits(Cm.next)):#x}, flagged {Cm.flagged} why {Cm.why}")
                assert n == Cm.hits, (what, "hit count", n, Cm.hits)
                docs = res[tag + "1doc"][i, :n]; sb = res[tag + "1score"][i, :n]
                bad = np.flatnonzero((docs != Cm.docs) | (sb != Cm.bits))
                assert not len(bad), (what, "rows", len(bad), [(int(j), int(docs[j]), hex(int(sb[j])), int(Cm.docs[j]), hex(int(Cm.bits[j]))) for j in bad[:6]])
                assert int(res[tag + "1next"][i]) == int(SM.bits(Cm.next)), (what, "next", hex(int(res[tag + "1next"][i])), hex(int(SM.bits(Cm.next))))
                # 2. the host's rule, no flags: the same bytes
                assert int(res[tag + "2hc"][i]) == n and np.array_equal(res[tag + "2doc"][i], res[tag + "1doc"][i]) and np.array_equal(res[tag + "2score"][i], res[tag + "1score"][i]), (what, "entry point 2")
                # 3. the replay on
                n3 = int(res[tag + "3hc"][i])
                if not Cm.flagged:
                    assert n3 == n and np.array_equal(res[tag + "3doc"][i], res[tag + "1doc"][i]) and np.array_equal(res[tag + "3score"][i], res[tag + "1score"][i]), (what, "entry point 3, not flagged")
                else:
                    why[Cm.why] += 1
                    got = dict(zip(res[tag + "3doc"][i, :n3].tolist(), res[tag + "3score"][i, :n3].tolist()))
                    assert n3 == len(R) == len(got), (what, "replay: hit count", n3, len(R))
                    assert set(got) == set(R), (what, "replay: documents", sorted(set(got) - set(R))[:8], sorted(set(R) - set(got))[:8])
                    wrong = [(d, hex(got[d]), hex(R[d])) for d in R if got[d] != R[d]]
                    assert not wrong, (what, "replay: score bits", len(wrong), wrong[:6])
            assert st["replays"] == why[0] + why[1], (setting, tag, "replays", st, why)
            assert st["why"] == [why[0], why[1], 0], (setting, tag, "why3", st, why)
            flagged_total[0] += why[0]; flagged_total[1] += why[1]
    print(f"{setting}: {secs:.1f} s; {len(BATCHES) * 2} batches, every cut exact; flagged over all batches: {flagged_total[0]} for an exact plateau, {flagged_total[1]} inside the band")
    if setting != SETTINGS[0]:                            # the same bytes whatever ran in front of k_select
        base = run_child(SETTINGS[0], tmp)[0]
        assert sorted(base) == sorted(res)
        for k in base:
            assert np.array_equal(base[k], res[k]), (setting, k)
