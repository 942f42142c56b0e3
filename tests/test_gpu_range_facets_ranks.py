"""range_facets across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted
flags, so each counts over the whole corpus on its own GPU — ShardedSearcher.range_facets needs no collective and must return, on every rank, what the
unsharded engine returns for the same requests, before and after a deletion.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
GONE = sorted(set(range(0, D, 7)) | {D - 1})


def requests():
    from infidex_amd import RangeRequest
    return [RangeRequest("year >= 2000 AND rating > 7.0", "rating", (float("-inf"), 7.0, 8.0, 9.0, float("inf"))), RangeRequest("block >= 16", "block", (0, 16, 17, 18)),
            RangeRequest(None, "year", tuple(range(1900, 2040, 10)))]


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
from tests.test_gpu_range_facets_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.range_facets(requests())
stats = [ss.last_range_stats()]
one = ss.range_facets("block >= 16", "block", (0, 16, 17, 18))
stats.append(ss.last_range_stats())
eng.delete_documents(GONE)
dead = ss.range_facets(requests())
stats.append(ss.last_range_stats())
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
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29658", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.range_facets(reqs)
    e.delete_documents(GONE)
    want_dead = e.range_facets(reqs)
    assert all(w.error is None and w.nan + w.below + sum(w.counts) + w.above == w.total for w in want_live + want_dead)
    assert want_live[0].total and want_live[0].below == 0 and want_live[0].counts[0] == 0               # rating > 7.0 only
    assert want_live[1].total == D - 65536 == want_live[1].counts[1] + want_live[1].counts[2] and want_live[1].min == 16 and want_live[1].max == 17      # rank 1's side of the corpus
    assert want_live[2].total == D and want_dead[2].total == D - len(GONE) and want_dead[1].total < want_live[1].total
    for r in range(2):
        live, one, dead, stats = got[r]
        assert live == want_live and dead == want_dead, r
        assert one == live[1]
        assert stats == [(2, 0, 1), (0, 1, 1), (2, 0, 1)], (r, stats)
