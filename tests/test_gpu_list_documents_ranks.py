"""list_documents across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global
Deleted flags, so each selects the page over the whole corpus on its own GPU — ShardedSearcher.list_documents needs no collective and must return, on
every rank, what the unsharded engine returns for the same requests, with deletions.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
GONE = sorted(set(range(0, D, 7)) | {D - 1})


def requests():
    from infidex_amd import ListRequest
    return [ListRequest("year >= 2000 AND rating > 7.0", "rating", False, 100, 64), ListRequest("block >= 16", "genre", True, 0, 1024), ListRequest(None, "year", True, 65500, 97),
            ListRequest("block IN (15, 16) AND year < 1960", "block", True, 0, 1024), ListRequest("year < 1900", "year"), ListRequest("rating = 7 OR year = ", "year"),
            ListRequest(None, None, True, 65530, 20), ListRequest("genre IN ('Drama', 'crime') OR year < 1960", "year", False, D, 5), ListRequest("block >= 0", "nosuch")]


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
from tests.test_gpu_list_documents_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.list_documents(requests())
stats = [ss.last_list_stats()[:2]]
one = ss.list_documents("block >= 16", "genre", True, 0, 1024)
stats.append(ss.last_list_stats()[:2])
eng.delete_documents(GONE)
dead = ss.list_documents(requests())
stats.append(ss.last_list_stats()[:2])
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
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29657", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.list_documents(reqs)
    e.delete_documents(GONE)
    want_dead = e.list_documents(reqs)
    assert want_live[0].total and len(want_live[1].document_ids) == 1024 and min(want_live[1].document_ids) >= 65536 and want_live[4].total == 0
    assert want_live[5].error and want_live[8].error and want_live[7].document_ids == [] and want_live[7].total
    assert want_live[6].document_ids == list(range(65530, 65550)) and want_dead[2].total == D - len(GONE)
    for r in range(2):
        live, one, dead, stats = got[r]
        assert live == want_live and dead == want_dead, r
        assert one == live[1]
        assert stats == [(5, 0), (0, 1), (5, 0)], (r, stats)
