"""The HIP streams a session creates, and that the replay gives the same rows wherever its k_ex_chunk launches run.

The runtime serves streams from a small pool of hardware queues (4 by default); streams beyond the pool share a queue and their kernels run one after the
other.  A session therefore keeps its hot path on ONE normal-priority stream (one of the main streams its index created up front); the replay's
side-by-side k_ex_chunk launches (a second normal-priority stream) are an opt-in, INFX_REPLAY_AUX=1, read when the library creates its first stream:
each mode runs in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import ctypes as C, sys, threading, numpy as np
from infidex_amd import SearchEngine
from infidex_amd.engine import Session, pack_texts
from tools.synth import Synth
s = Synth(2, docs=180000); arena, offs = s.docs()
e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
qa, qo = s.queries(200, qseed=21, fuzz=0.3)
a, o = pack_texts(Synth.texts(qa, qo))
sessions = [Session(e) for _ in range(4)]
budget = []
for se in sessions:
    n, h = C.c_int32(-1), C.c_int32(-1)
    e._check(e.L.infx_engine_session_stream_budget(se.h, C.byref(n), C.byref(h)))
    budget.append((n.value, h.value))
def native(fn, h):
    p = C.c_void_p()
    e._check(fn(h, C.byref(p)))
    return int(p.value or 0)
own = native(e.L.infx_engine_stream_native, e.h)
mains = [native(e.L.infx_engine_session_stream_native, se.h) for se in sessions]
one = sessions[0].search_packed(a, o, 10, 500)
replays = sessions[0].last_timings()["exact_replays"]
# four sessions at once on the one index, three rounds each, and the engine's own session beside them (a fifth user: it shares a main stream with one of
# the four): every call must return what the single session returned
users = sessions + [e]
outs = [[None] * 3 for _ in users]; errs = []
def work(i):
    try:
        for r in range(3):
            outs[i][r] = users[i].search_packed(a, o, 10, 500)
    except Exception as ex:
        errs.append(ex)
ths = [threading.Thread(target=work, args=(i,)) for i in range(len(users))]
for t in ths: t.start()
for t in ths: t.join()
if errs: raise errs[0]
same = all(np.array_equal(x, y) for per in outs for got in per for x, y in zip(got, one))
k, sc, t, c, f = one
np.savez(sys.argv[1], k=k, sc=sc, t=t, c=c, f=f, budget=np.asarray(budget, np.int64), own=np.uint64(own), mains=np.asarray(mains, np.uint64), replays=np.int64(replays), same=np.int64(same))
'''


def run_mode(tmp_path, aux):
    env = dict(os.environ); env.pop("INFX_REPLAY_AUX", None); env.pop("INFX_MAIN_STREAMS", None)
    if aux is not None:
        env["INFX_REPLAY_AUX"] = aux
    env["PYTHONPATH"] = ROOT
    out = str(tmp_path / f"aux_{aux}.npz")
    subprocess.run([sys.executable, "-c", SCRIPT, out], check=True, env=env, cwd=ROOT, timeout=900)
    return np.load(out)


@pytest.fixture(scope="module")
def modes(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_budget")
    return run_mode(d, None), run_mode(d, "1")


def test_default_session_has_one_normal_priority_stream(modes):
    default, aux = modes
    print("streams per session (normal, high): default", default["budget"].tolist(), "INFX_REPLAY_AUX=1", aux["budget"].tolist())
    assert [int(n) for n, _ in default["budget"]] == [1, 1, 1, 1]
    assert [int(n) for n, _ in aux["budget"]] == [2, 2, 2, 2]
    for b in (default["budget"], aux["budget"]):
        assert all(0 <= int(h) <= 1 for _, h in b)       # the planning stream, where the device offers stream priorities
    assert default["budget"][:, 1].tolist() == aux["budget"][:, 1].tolist()


def test_replayed_queries_are_the_same_in_both_modes(modes):
    default, aux = modes
    print("replayed queries of the batch: default", int(default["replays"]), "INFX_REPLAY_AUX=1", int(aux["replays"]))
    assert int(default["replays"]) > 0 and int(default["replays"]) == int(aux["replays"])      # the batch really holds flagged queries
    for key in ("k", "sc", "t", "c", "f"):
        assert np.array_equal(default[key], aux[key]), key


def test_four_concurrent_sessions_return_what_one_returns(modes):
    for m in modes:
        assert int(m["same"]) == 1


def test_sessions_draw_distinct_main_streams_from_the_pool(modes):
    """The engine's own session and four sessions on the default pool of four main streams: four distinct streams, and the only one with two users is the
    engine's own (created first, idle once sessions run)."""
    for m in modes:
        own, mains = int(m["own"]), [int(x) for x in m["mains"]]
        print("main streams: engine's own session %#x, sessions %s" % (own, [hex(x) for x in mains]))
        assert own != 0 and all(x != 0 for x in mains)
        assert len(set(mains)) == 4                          # no two sessions on one stream
        assert len(set(mains + [own])) == 4                  # a pool of four: the fifth user shares
        assert mains.count(own) == 1 and mains[3] == own     # ... the engine's own stream, with the fourth session
