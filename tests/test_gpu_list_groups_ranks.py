"""list_groups across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted
flags, so each finds the heads and selects the page over the whole corpus on its own GPU — ShardedSearcher.list_groups needs no collective and must return,
on every rank, what the unsharded engine returns for the same requests, with deletions.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest;
the groups of `block` 16 lie wholly on rank 1's side, the groups of `year`, `genre` and `rating` span both."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
GONE = sorted(set(range(0, D, 7)) | {D - 1})


def requests():
    from infidex_amd import GroupListRequest
    return [GroupListRequest("year >= 2000 AND rating > 7.0", "genre", "rating", False, 0, 64), GroupListRequest("block >= 16", "year", "genre", True, 3, 1024),
            GroupListRequest(None, "block", "year", True, 0, 97), GroupListRequest(None, "block", "year", True, 15, 97), GroupListRequest(None, "rating", None, True, 40, 20),
            GroupListRequest("year < 1900", "year", "year"), GroupListRequest("rating = 7 OR year = ", "year", "year"), GroupListRequest(None, "year", None, False, D, 5),
            GroupListRequest("block >= 0", "nosuch", "year"), GroupListRequest("block IN (15, 16) AND year < 1960", "block", "rating", False, 0, 1024)]


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
from tests.test_gpu_list_groups_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.list_groups(requests())
stats = [ss.last_group_list_stats()[:3]]
one = ss.list_groups("block >= 16", "year", "genre", True, 3, 1024)
stats.append(ss.last_group_list_stats()[:3])
eng.delete_documents(GONE)
dead = ss.list_groups(requests())
stats.append(ss.last_group_list_stats()[:3])
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
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29660", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.list_groups(reqs)
    e.delete_documents(GONE)
    want_dead = e.list_groups(reqs)
    assert want_live[0].total and want_live[0].total_groups == len(want_live[0].document_ids) > 3
    assert want_live[1].total == D - 65536 and min(want_live[1].document_ids) >= 65536 and sum(want_live[1].group_sizes) < want_live[1].total      # (offset 3)
    assert want_live[2].total_groups == 18 and want_live[2].group_values[:3] != [] and sum(want_live[2].group_sizes) == D and want_live[3].group_values == want_live[2].group_values[15:]
    assert want_live[5].total == 0 and want_live[5].total_groups == 0 and want_live[6].error and want_live[8].error and "nosuch" in want_live[8].error
    assert want_live[7].document_ids == [] and want_live[7].total == D and want_live[7].total_groups > 50
    assert want_dead[2].total == D - len(GONE) and sum(want_dead[2].group_sizes) == D - len(GONE)
    for r in range(2):
        live, one, dead, stats = got[r]
        assert live == want_live and dead == want_dead, r
        assert one == live[1]
        # four distinct filters in the call (None needs no mask); requests 2 and 3 are pages of one listing: seven head passes for eight answered requests
        assert stats == [(4, 0, 7), (0, 1, 1), (4, 0, 7)], (r, stats)
