"""field_quantiles across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted
flags, so each selects over the whole corpus on its own GPU — ShardedSearcher.field_quantiles needs no collective and must return, on every rank, what
the unsharded engine returns for the same requests, before and after a deletion.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest."""
import math
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
GONE = sorted(set(range(0, D, 7)) | {D - 1})
BOX = (0, 0.25, 0.5, 0.75, 1)


def requests():
    from infidex_amd import QuantileRequest
    return [QuantileRequest("year >= 2000 AND rating > 7.0", "rating", BOX, "genre"), QuantileRequest("block >= 16", "block", (0.5, 0.0, 1.0), "block"),
            QuantileRequest(None, "year", (0.999, 1 / 3)), QuantileRequest(None, "rating", (0.5,), "year")]


def engine_columns(eng):
    from tests.test_gpu_filtered_facets_ranks import engine_columns as base
    base(eng)


RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_field_quantiles_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.field_quantiles(requests())
stats = [ss.last_field_quantiles_stats()[:2]]
one = ss.field_quantiles("block >= 16", "block", (0.5, 0.0, 1.0), "block")
stats.append(ss.last_field_quantiles_stats()[:2])
eng.delete_documents(GONE)
dead = ss.field_quantiles(requests())
stats.append(ss.last_field_quantiles_stats()[:2])
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((live, one, dead, stats), f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_the_unsharded_engine(tmp_path):
    import numpy as np
    from infidex_amd import SearchEngine
    from tests.test_gpu_boost_sort import columns
    from tools.synth import Synth
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29661", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.field_quantiles(reqs)
    e.delete_documents(GONE)
    want_dead = e.field_quantiles(reqs)
    assert all(w.error is None and w.count + w.nan == w.total == sum(g.count + g.nan for g in w.groups or [w]) for w in want_live + want_dead)
    # the unsharded engine itself against the columns' values
    year, rating, _ = columns(D)
    y = np.sort(np.asarray(year, np.int64))
    assert want_live[2].total == D and want_live[2].values == [int(y[math.floor((D - 1) * 0.999)]), int(y[math.floor((D - 1) * (1 / 3))])] and want_dead[2].total == D - len(GONE)
    r = np.asarray(rating, np.float64); fin = np.sort(r[~np.isnan(r)])
    assert want_live[3].values == [float(fin[(len(fin) - 1) // 2])] and want_live[3].count == len(fin) and want_live[3].count + want_live[3].nan == D
    assert want_live[1].total == D - 65536 and want_live[1].values == [16, 16, 17] and [(g.value, g.values) for g in want_live[1].groups] == [("16", [16] * 3), ("17", [17] * 3)]      # rank 1's side of the corpus
    assert want_dead[1].total < want_live[1].total
    for rk in range(2):
        live, one, dead, stats = got[rk]
        assert live == want_live and dead == want_dead, rk
        assert one == live[1]
        assert stats == [(2, 0), (0, 1), (2, 0)], (rk, stats)
