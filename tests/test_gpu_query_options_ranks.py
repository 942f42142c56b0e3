"""Per-query options across two real ranks (two processes, torch.distributed gloo, both on GPU 0): ShardedSearcher.search_queries must return, row
for row, facet for facet and count for count, what the unsharded engine returns for the same mixed batch (tests/test_gpu_query_options.py).
NumberOfDocumentsInFilter is the whole corpus's on every rank, with no collective."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_boost_sort import columns
from tests.test_gpu_query_options import mixed_queries
from tools.synth import Synth
s = Synth(2, docs=40000); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
year, rating, genre = columns(40000)
eng.set_column("year", year, facetable=True); eng.set_column("rating", rating, facetable=False); eng.set_column("genre", genre, facetable=True)
qa, qo = s.queries(60, qseed=43, fuzz=0.3)
qs = mixed_queries(Synth.texts(qa, qo), n=96, seed=5)
res = ShardedSearcher(eng, TorchComm(dist)).search_queries(qs)
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump(res, f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_unsharded(tmp_path):
    from infidex_amd import SearchEngine
    from tests.test_gpu_boost_sort import columns
    from tests.test_gpu_query_options import mixed_queries, assert_same
    from tools.synth import Synth
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29643", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=40000); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    year, rating, genre = columns(40000)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    qa, qo = s.queries(60, qseed=43, fuzz=0.3)
    qs = mixed_queries(Synth.texts(qa, qo), n=96, seed=5)
    want = e.search_queries(qs)
    for r in range(2):
        for q, a, w in zip(qs, got[r], want):
            assert_same(a, w, (r, q.text, q.filter))
