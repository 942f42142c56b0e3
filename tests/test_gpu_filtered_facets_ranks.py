"""facets_of_documents across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the
global Deleted flags, so each evaluates the filters over the whole corpus on its own GPU — ShardedSearcher.facets_of_documents needs no collective
and must return, on every rank, the model's answer (tests/test_gpu_filtered_facets.py: the oracle's filter VM per document and plain counting),
with deletions.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
EXPRS = ["year >= 2000 AND rating > 7.0", "genre IN ('Drama', 'crime') OR year < 1960", "block >= 16", "block < 16 AND genre = 'Drama'", "year < 1900",
         "block >= 0", "block IN (15, 16) AND year < 1960", "rating = 7 OR year = ", "year BETWEEN 1990 AND 1999"]
GONE = sorted(set(range(0, D, 7)) | {D - 1})


def engine_columns(eng):
    import numpy as np
    from tests.test_gpu_boost_sort import columns
    year, rating, genre = columns(D)
    eng.set_column("year", year, facetable=True); eng.set_column("rating", rating, facetable=False); eng.set_column("genre", genre, facetable=True)
    eng.set_column("block", np.arange(D, dtype=np.int64) // 4096, facetable=False)      # block 16 begins at document 65 536: rank 1's side


RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_filtered_facets_ranks import engine_columns, D, EXPRS, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.facets_of_documents(EXPRS)
stats = [ss.last_filtered_facet_stats()]
one = ss.facets_of_documents(EXPRS[0])
stats.append(ss.last_filtered_facet_stats())
eng.delete_documents(GONE)
dead = ss.facets_of_documents(EXPRS)
stats.append(ss.last_filtered_facet_stats())
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((live, one, dead, stats), f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_the_model(tmp_path):
    import numpy as np
    from tests.test_gpu_boost_sort import columns
    from tests.test_gpu_filtered_facets import FilteredModel
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29653", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    year, rating, genre = columns(D)
    m = FilteredModel({"year": (year, True), "rating": (rating, False), "genre": (genre, True), "block": (np.arange(D, dtype=np.int64) // 4096, False)})
    bad = EXPRS.index("rating = 7 OR year = ")
    for r in range(2):
        live, one, dead, stats = got[r]
        assert stats == [(len(EXPRS) - 1, 0, 1), (0, 1, 0), (len(EXPRS) - 1, 0, 1)], (r, stats)
        assert one == live[0]
        for state, deleted in ((live, []), (dead, GONE)):
            m.set_deleted(deleted)
            for i, (x, g) in enumerate(zip(EXPRS, state)):
                if i == bad:
                    assert g.error and g.facets == {} and g.total == 0, r
                else:
                    m.check(g, x, (r, bool(deleted)))
        assert live[2].total == D - 65536 and dead[5].total == D - len(GONE)
    assert got[0][0] == got[1][0] and got[0][2] == got[1][2]
