"""list_group_members across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted
flags, so each finds the heads, selects the page and walks the set for the members over the whole corpus on its own GPU —
ShardedSearcher.list_group_members needs no collective and must return, on every rank, what the unsharded engine returns for the same requests, with
deletions.  The corpus and the columns are tests/test_gpu_list_groups_ranks.py's: 70 000 documents, rank 0 owns the first 65 536, rank 1 the rest; the groups
of `block` 16 lie wholly on rank 1's side, the groups of `year`, `genre` and `rating` span both."""
import os
import pickle
import subprocess
import sys

import pytest

from tests.test_gpu_list_groups_ranks import engine_columns, D, GONE      # noqa: F401 (engine_columns: used by the rank script through this module)

pytestmark = pytest.mark.gpu


def requests():
    from infidex_amd import GroupMembersRequest as M
    return [M("year >= 2000 AND rating > 7.0", "genre", "rating", False, 3, 0, 64), M("block >= 16", "year", "genre", True, 2, 3, 1024), M(None, "block", "year", True, 16, 0, 97),
            M(None, "block", "year", True, 1, 15, 97), M(None, "rating", None, True, 5, 40, 20), M("year < 1900", "year", "year"), M("rating = 7 OR year = ", "year", "year"),
            M(None, "year", None, False, 3, D, 5), M("block >= 0", "nosuch", "year"), M("block IN (15, 16) AND year < 1960", "block", "rating", False, 4, 0, 1024),
            M(None, "year", "rating", True, 17)]


RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_group_members_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.list_group_members(requests())
stats = [ss.last_group_members_stats()[:3]]
one = ss.list_group_members("block >= 16", "year", "genre", True, 2, 3, 1024)
stats.append(ss.last_group_members_stats()[:3])
eng.delete_documents(GONE)
dead = ss.list_group_members(requests())
stats.append(ss.last_group_members_stats()[:3])
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((live, one, dead, stats), f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_the_unsharded_engine(tmp_path):
    from infidex_amd import SearchEngine, GroupListRequest
    from tools.synth import Synth
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29664", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.list_group_members(reqs)
    heads_live = e.list_groups([GroupListRequest(r.filter, r.group_by, r.order_by, r.ascending, r.offset, r.limit) for r in reqs[:10]])
    e.delete_documents(GONE)
    want_dead = e.list_group_members(reqs)
    for m, h in zip(want_live, heads_live):                                   # the unsharded answer is list_groups' with members behind the heads
        assert (m.error is None) == (h.error is None)
        assert ([g.document_ids[0] for g in m.groups], [g.size for g in m.groups], m.total_groups, m.total) == (h.document_ids, h.group_sizes, h.total_groups, h.total)
    assert want_live[0].total and all(len(g.document_ids) == min(3, g.size) for g in want_live[0].groups) and len(want_live[0].groups) > 3
    assert want_live[1].total == D - 65536 and min(d for g in want_live[1].groups for d in g.document_ids) >= 65536
    assert len(want_live[2].groups) == 18 and all(len(g.document_ids) == 16 for g in want_live[2].groups) and sum(g.size for g in want_live[2].groups) == D
    assert want_live[5].total == 0 and want_live[5].groups == [] and want_live[6].error and want_live[8].error and "nosuch" in want_live[8].error
    assert want_live[7].groups == [] and want_live[7].total == D and want_live[7].total_groups > 50 and want_live[10].error and "per_group" in want_live[10].error
    assert want_dead[2].total == D - len(GONE) and sum(g.size for g in want_dead[2].groups) == D - len(GONE)
    assert not set(GONE) & {d for g in want_dead[2].groups for d in g.document_ids}
    for r in range(2):
        live, one, dead, stats = got[r]
        assert live == want_live and dead == want_dead, r
        assert one == live[1]
        # four distinct filters in the call (None needs no mask); requests 2 and 3 differ in per_group only and are pages of one listing: seven head passes
        assert stats == [(4, 0, 7), (0, 1, 1), (4, 0, 7)], (r, stats)
