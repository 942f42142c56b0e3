"""field_distinct across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted
flags, so each marks and counts over the whole corpus on its own GPU — ShardedSearcher.field_distinct needs no collective and must return, on every rank,
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
    from infidex_amd import DistinctRequest
    return [DistinctRequest("year >= 2000 AND rating > 7.0", "rating", "genre"), DistinctRequest("block >= 16", "block", "block"), DistinctRequest(None, "year", None),
            DistinctRequest(None, "uniq", "genre"), DistinctRequest("block >= 16", "uniq", "year"), DistinctRequest(None, "genre", "year")]


def engine_columns(eng):
    from tests.test_gpu_top_groups_ranks import engine_columns as base      # (the columns of the filtered-facet ranks test and a unique column)
    base(eng)


RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_field_distinct_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.field_distinct(requests())
stats = [ss.last_field_distinct_stats()[:2]]
one = ss.field_distinct("block >= 16", "block", "block")
stats.append(ss.last_field_distinct_stats()[:2])
eng.delete_documents(GONE)
dead = ss.field_distinct(requests())
stats.append(ss.last_field_distinct_stats()[:2])
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((live, one, dead, stats), f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_the_unsharded_engine(tmp_path):
    from infidex_amd import SearchEngine
    from tools.synth import Synth
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29663", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.field_distinct(reqs)
    # the unsharded engine itself against list_groups and field_stats
    for r, w in zip(reqs, want_live):
        assert w.error is None and w.distinct == e.list_groups(r.filter, r.field).total_groups and w.total == e.list_documents(r.filter).total, r
    st = e.field_stats("block >= 16", "year", "year")
    assert [(g.value, g.size) for g in want_live[4].groups] == [(g.value, g.count) for g in st.groups] and all(g.distinct == g.size for g in want_live[4].groups)
    assert [(g.value, g.distinct) for g in want_live[1].groups] == [("16", 1), ("17", 1)] and want_live[1].distinct == 2 and want_live[1].total == D - 65536      # rank 1's side
    assert want_live[3].distinct == want_live[3].total == D
    e.delete_documents(GONE)
    want_dead = e.field_distinct(reqs)
    assert all(w.error is None for w in want_dead) and want_dead[3].distinct == D - len(GONE) and want_dead[1].total < want_live[1].total
    for rk in range(2):
        live, one, dead, stats = got[rk]
        assert live == want_live and dead == want_dead, rk
        assert one == live[1]
        assert stats == [(2, 0), (0, 1), (2, 0)], (rk, stats)
