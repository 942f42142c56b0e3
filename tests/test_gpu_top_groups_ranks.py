"""top_groups across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted flags,
so each accumulates, ranks and selects over the whole corpus on its own GPU — ShardedSearcher.top_groups needs no collective and must return, on every rank,
what the unsharded engine returns for the same requests, before and after a deletion.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
GONE = sorted(set(range(0, D, 7)) | {D - 1})


def requests():
    from infidex_amd import TopGroupsRequest
    return [TopGroupsRequest("year >= 2000 AND rating > 7.0", "genre", "mean", "rating", False, 0, 20), TopGroupsRequest("block >= 16", "block", "sum", "block", True, 0, 5),
            TopGroupsRequest(None, "year", "size", None, False, 3, 10), TopGroupsRequest(None, "uniq", "max", "rating", False, 69000, 1024),
            TopGroupsRequest("block >= 16", "uniq", "sum", "year", True, 4000, 1024), TopGroupsRequest(None, "year", "min", "rating", True, 0, 1024)]


def engine_columns(eng):
    import numpy as np
    from tests.test_gpu_filtered_facets_ranks import engine_columns as base
    base(eng)
    eng.set_column("uniq", np.arange(D, dtype=np.int64) * 3 + 1, facetable=False)      # every document its own group: 70 000 slots


RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_top_groups_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.top_groups(requests())
stats = [ss.last_top_groups_stats()[:3]]
one = ss.top_groups("block >= 16", "block", "sum", "block", True, 0, 5)
stats.append(ss.last_top_groups_stats()[:3])
eng.delete_documents(GONE)
dead = ss.top_groups(requests())
stats.append(ss.last_top_groups_stats()[:3])
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((live, one, dead, stats), f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_the_unsharded_engine(tmp_path):
    from infidex_amd import SearchEngine, StatsRequest
    from tools.synth import Synth
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29662", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.top_groups(reqs)
    # the unsharded engine itself against field_stats, where that can answer
    st = e.field_stats([StatsRequest(r.filter, r.field, r.group_by) for r in (reqs[0], reqs[1])])
    assert sorted((g.value, g.mean) for g in st[0].groups) == sorted((r.value, r.mean) for r in want_live[0].groups) and len(st[0].groups) <= 20
    assert [r.mean for r in want_live[0].groups] == sorted((r.mean for r in want_live[0].groups), reverse=True)
    assert [(r.value, r.sum) for r in want_live[1].groups] == [("17", 17 * (D - 65536 - 4096)), ("16", 16 * 4096)] and want_live[1].total == D - 65536      # rank 1's side, the smaller sum first
    assert want_live[3].total_groups == want_live[3].total == D and len(want_live[3].groups) == 1000 and len(want_live[4].groups) == D - 65536 - 4000
    e.delete_documents(GONE)
    want_dead = e.top_groups(reqs)
    assert all(w.error is None for w in want_live + want_dead) and want_dead[3].total_groups == D - len(GONE) and want_dead[1].total < want_live[1].total
    for rk in range(2):
        live, one, dead, stats = got[rk]
        assert live == want_live and dead == want_dead, rk
        assert one == live[1]
        assert stats == [(2, 0, 6), (0, 1, 1), (2, 0, 6)], (rk, stats)
