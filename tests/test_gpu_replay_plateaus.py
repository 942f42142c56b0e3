"""The exact Stage-1 replay (k_ex_walk, k_ex_prefix, k_ex_theta, k_ex_chunk<1|4|16>, k_ex_heap, and the fallback k_exact1) held to tests/replay_model.py through the
raw C ABI (include/infidex_hip.h), on the constructed index replay_model.PlateauIndex: 140 072 documents of four lengths, so that every query of
replay_model.plateau_batch has rows of bit-equal first-pass score on both sides of its cut and k_select flags it for an exact plateau.  No text, no oracle:
tests/test_replay_model.py pins the model to the oracle on the CPU and shows that each named query is the plateau it says and that the batch tells five misreadings
of the reference from the right one.

One child process per (range width, replay variant) — widths 512, the default (range_docs 0: 1024 at this size) and 16384, i.e. 128, 64 and 4 ranges per 65 536-id
container in k_ex_walk; variants: the environment unset (parallel kernels, heap in registers), INFX_EXACT_SLOW=1 (k_exact1 for every flagged query) and
INFX_EX_HEAP_LDS=1 (parallel kernels, heap in LDS).  The variables are read once per process; children run one after the other, each under its own time limit, and
once one ends abnormally (a signal, an abort, its time limit) no further child is started.  A child runs one batch per depth of replay_model.DEPTHS (1, 2, 63, 64, 65,
500, 512 on an index of max_depth 512; 513 and 1024 on one of max_depth 1024, where k_exact1 takes every flagged query), before and after infx_set_deleted, in batches
of one, two and four mask words (the 40-term and the 70-term query added in turn; k_mark_wide hands the latter to k_exact1).

Held for every query, with nothing excused:
  - infx_stage1_select's hit count, the returned documents and every score's fp32 bits are the model's;
  - infx_last_exact_replays and infx_last_replay_stats' why3[0] equal the batch's query count: every query was flagged, and for an exact plateau;
  - the rows of one width are byte-identical across the three variants (heap array order included);
  - with the environment unset, at depth <= 512, the queries handed to k_exact1 (infx_last_exact_fallbacks) stay below the batch's query count, and in a batch
    without the 70-term query they are printed per child: the parallel kernels, not the fallback, produced most of what is compared.

Nothing in the batch but "refused interval" makes k_ex_heap refuse a chunk's threshold interval: with real maxScore bounds the exact and the predicted threshold
differ by an ulp at most here and no candidate's bound falls between them.  That query hands REFB a maxScore that adds nothing to the running score, so that at
depths 1 and 2 the two thresholds decide REFB's tail rows differently and k_ex_heap must hand the query to k_exact1 (replay_model.plateau_batch says how).

First run on an MI355X (17 queries in the widest batch, 108 batches per child): every child passed, nothing excused.  Replays per batch: all of its queries (15, 16
and 17 at the three batch widths), each flagged for an exact plateau.  Handed to k_exact1 by the parallel replay, in the 36 batches per child without the 70-term
query: 8 queries (one per batch at depths 1 and 2: "refused interval") with the environment unset and with INFX_EX_HEAP_LDS=1, at every width; none elsewhere; with
INFX_EXACT_SLOW=1 the parallel replay does not run.  Wall time per child: 1.1 - 1.2 s at widths 512 and default, 2.2 - 2.4 s at 16384; CHILD_TIMEOUT is ten times
the slowest, a stall guard.  Tried once by hand: with the interval test taken out of k_ex_heap, "refused interval" fails at depth 1 (a tail row of container 1
is returned in place of container 0's first row)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import replay_model as RM

pytestmark = pytest.mark.gpu
WIDTHS = (512, 0, 16384)
VARIANTS = (None, "INFX_EXACT_SLOW", "INFX_EX_HEAP_LDS")
CHILD_TIMEOUT = 25

CHILD = r'''
import ctypes as C, json, sys
import numpy as np
from infidex_amd.engine import load_library, _p
from tests.test_gpu_device_abi import Cfg, Term, Query, Hit, chk
from tests import replay_model as RM, stage1_model as M
R, out = int(sys.argv[1]), sys.argv[2]
L = load_library()
P = RM.PlateauIndex(); N = P.N
f32 = np.float32
res, stats = {}, {}
for cap in (512, 1024):
    depths = [d for d in RM.DEPTHS if (d <= 512) == (cap == 512)]
    idx = C.c_void_p(); st = C.c_void_p()
    cfg = Cfg(0, R, cap, 0)
    chk(L, L.infx_create(C.byref(cfg), C.byref(idx)))
    keys = np.arange(N, dtype=np.int64)
    chk(L, L.infx_upload_docs(idx, N, _p(P.doc_len, C.c_float), C.c_float(P.avgdl), _p(keys, C.c_int64), None, None, None))
    chk(L, L.infx_upload_postings(idx, P.T, _p(P.post_off, C.c_uint64), _p(P.post_doc, C.c_int32), _p(P.post_w, C.c_uint8), _p(P.df, C.c_int32)))
    chk(L, L.infx_stream_create(idx, C.byref(st)))
    for deleted in (0, 1):
        if deleted:
            flagsN = np.zeros(N, np.uint8); flagsN[P.gone] = 1
            chk(L, L.infx_set_deleted(idx, N, _p(flagsN, C.c_uint8)))
        for depth in depths:
            for level in (0, 1, 2):
                qs, terms, extra = [], [], []
                for Q in RM.plateau_batch(P, level):
                    ix, mt, pl, bounds = RM.plateau_model(P, Q, depth)
                    ids = ([-1] if Q["virt"] else []) + [P.id[n] for n in Q["terms"]]
                    qs.append(Query(len(terms), len(ids), pl.mode, -1, depth, pl.n_and, pl.df_s1, pl.df_s2))
                    for t, tid, role, rank, mx in zip(mt, ids, pl.roles, pl.ranks, bounds):
                        idf = float(t.idf); mx = float(mx)
                        if tid >= 0: terms.append(Term(tid, 0, 0, idf, mx, role, rank, 0))
                        else: terms.append(Term(-1, len(extra), len(t.docs), idf, mx, role, rank, 0)); extra += t.docs.tolist()     # the caller's union
                nq = len(qs)
                QA = (Query * nq)(*qs); TA = (Term * len(terms))(*terms); EX = np.asarray(extra, np.int32)
                counts = np.zeros((nq, M.NCLASS), np.uint32)
                chk(L, L.infx_stage1_accumulate(st, nq, QA, len(terms), TA, len(EX), _p(EX, C.c_int32), counts.ctypes.data_as(C.c_void_p)))
                hits = (Hit * (nq * depth))(); hc = np.zeros(nq, np.uint32)
                chk(L, L.infx_stage1_select(st, nq, counts.ctypes.data_as(C.c_void_p), hits, _p(hc, C.c_uint32)))
                h = np.frombuffer(hits, dtype=[("doc", np.int32), ("score", np.uint32)]).reshape(nq, depth).copy()
                for i in range(nq): h[i, int(hc[i]):] = 0
                n = C.c_uint32(0); fb = C.c_uint32(0); ms = C.c_float(0); why = (C.c_uint32 * 3)(); ms4 = (C.c_float * 4)()
                chk(L, L.infx_last_exact_replays(st, C.byref(n))); chk(L, L.infx_last_exact_fallbacks(st, C.byref(fb)))
                chk(L, L.infx_last_replay_stats(st, C.byref(ms), why)); chk(L, L.infx_last_replay_breakdown(st, ms4))
                tag = "d%d_k%d_l%d_" % (deleted, depth, level)
                res[tag + "hc"] = hc; res[tag + "doc"] = h["doc"]; res[tag + "score"] = h["score"]
                stats[tag] = dict(nq=nq, replays=int(n.value), fallbacks=int(fb.value), why=[int(x) for x in why], ms=float(ms.value), exact1_ms=float(ms4[3]))
    L.infx_stream_destroy(st); L.infx_destroy(idx)
np.savez(out, **res)
print("STATS " + json.dumps(stats))
'''

_stop = []          # why nothing more is started on the GPU
_runs = {}
_model = {}


def run_child(R, variant, tmp):
    key = (R, variant)
    if key in _runs:
        return _runs[key]
    if _stop:
        pytest.fail("no further child is started: " + _stop[0])
    env = dict(os.environ)
    for v in VARIANTS[1:]:
        env.pop(v, None)
    if variant is not None:
        env[variant] = "1"
    env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp / f"plateaus_{R}_{variant}.npz")
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, str(R), out], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _stop.append(f"the child of R = {R}, {variant} ran into its time limit")
        pytest.fail(_stop[0])
    if p.returncode != 0:
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            _stop.append(f"the child of R = {R}, {variant} ended abnormally ({p.returncode})")
        pytest.fail(f"child R = {R}, {variant}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    stats = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("STATS "))[6:])
    _runs[key] = (dict(np.load(out)), stats, time.time() - t0)
    return _runs[key]


def model_of(P, depth, deleted):
    """Per query of the widest batch: (name, doc -> fp32 bits)."""
    if (depth, deleted) not in _model:
        per = []
        for Q in RM.plateau_batch(P, 2):
            ix, terms, pl, ms = RM.plateau_model(P, Q, depth, bool(deleted))
            per.append((Q["name"], RM.replay(ix, terms, pl.cand, depth, ms).result))
        _model[(depth, deleted)] = per
    return _model[(depth, deleted)]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("replay_plateaus")


@pytest.fixture(scope="module")
def plateau():
    return RM.PlateauIndex()


@pytest.mark.parametrize("variant", VARIANTS, ids=["default", "slow", "lds-heap"])
@pytest.mark.parametrize("R", WIDTHS, ids=["512", "default-width", "16384"])
def test_replay_kernels_against_the_model(R, variant, tmp, plateau):
    res, stats, secs = run_child(R, variant, tmp)
    P = plateau
    fallbacks = {}
    for deleted in (0, 1):
        for depth in RM.DEPTHS:
            model = model_of(P, depth, deleted)
            for level in (0, 1, 2):
                tag = f"d{deleted}_k{depth}_l{level}_"
                names = [Q["name"] for Q in RM.plateau_batch(P, level)]
                assert [m[0] for m in model][:len(names)] == names
                S = stats[tag]
                for i, (name, want) in enumerate(model[:len(names)]):
                    what = (R, variant, tag, name)
                    n = int(res[tag + "hc"][i])
                    docs = res[tag + "doc"][i, :n].tolist(); bits = res[tag + "score"][i, :n].tolist()
                    assert n == len(want), (what, "hit count", n, len(want))
                    got = dict(zip(docs, bits))
                    assert len(got) == n, (what, "a document twice")
                    assert set(got) == set(want), (what, "documents", len(set(got) ^ set(want)), sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
                    wrong = [(d, hex(got[d]), hex(want[d])) for d in want if got[d] != want[d]]
                    assert not wrong, (what, "score bits", len(wrong), wrong[:6])
                assert S["replays"] == S["nq"] == len(names), (R, variant, tag, "replayed", S)
                assert S["why"][0] == S["nq"], (R, variant, tag, "flagged for an exact plateau", S)
                if variant is None and depth <= 512:
                    assert S["fallbacks"] < S["nq"], (R, variant, tag, "every query fell back to k_exact1", S)
                if level < 2:
                    fallbacks[tag] = S["fallbacks"]
    nb = len(fallbacks)
    print(f"R = {R}, {variant}: {secs:.1f} s; {nb} batches of <= 64 terms, every query replayed and flagged for an exact plateau; handed to k_exact1 by the parallel "
          f"replay: {sum(fallbacks.values())} queries in all, at most {max(fallbacks.values())} of a batch "
          f"({ {k: v for k, v in fallbacks.items() if v} })")
    if variant is not None:                               # the same bytes whichever kernels replayed
        base = run_child(R, None, tmp)[0]
        assert sorted(base) == sorted(res)
        for k in base:
            assert np.array_equal(base[k], res[k]), (R, variant, k)
