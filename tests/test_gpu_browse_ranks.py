"""Browse queries across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global
Deleted flags, so each computes the browse rows of the whole corpus itself — ShardedSearcher.search_queries must return the unsharded results on
every rank, for browse queries interleaved with text queries, and facets_of_all_documents the unsharded facets.  70 000 documents: rank 0 owns the
first 65 536, rank 1 the rest, and several filters place their rows on rank 1's side of the boundary."""
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000


def batch(texts):
    from infidex_amd import Query
    from tests.test_gpu_browse import EXPRS, PLACED
    qs = []
    for i, x in enumerate([None] + EXPRS + PLACED):
        qs.append(Query("" if i % 2 else "  ", [1, 10, 64][i % 3], filter=x, enable_facets=True))
        if i % 3 == 0:
            qs.append(Query(texts[i % len(texts)], 10, filter=EXPRS[i % len(EXPRS)], enable_facets=i % 2 == 0, sort_by="year" if i % 4 == 0 else None))
    qs.append(Query("", 10))                                          # blank without facets: empty
    return qs


def engine_columns(eng):
    import numpy as np
    from tests.test_gpu_boost_sort import columns
    year, rating, genre = columns(D)
    eng.set_column("year", year, facetable=True); eng.set_column("rating", rating, facetable=False); eng.set_column("genre", genre, facetable=True)
    eng.set_column("pos", np.arange(D, dtype=np.int64), facetable=False)


RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests.test_gpu_browse_ranks import batch, engine_columns, D
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
qa, qo = s.queries(40, qseed=43, fuzz=0.3)
ss = ShardedSearcher(eng, TorchComm(dist))
res = ss.search_queries(batch(Synth.texts(qa, qo)))
allf = ss.facets_of_all_documents()
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((res, allf), f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_unsharded_and_the_model(tmp_path):
    import numpy as np
    from infidex_amd import SearchEngine
    from tests.browse_model import BrowseModel
    from tests.test_gpu_boost_sort import columns
    from tests.test_gpu_query_options import assert_same
    from tools.synth import Synth
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29647", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    year, rating, genre = columns(D)
    m = BrowseModel({"year": (year, True), "rating": (rating, False), "genre": (genre, True), "pos": (np.arange(D, dtype=np.int64), False)})
    qa, qo = s.queries(40, qseed=43, fuzz=0.3)
    qs = batch(Synth.texts(qa, qo))
    want = e.search_queries(qs)
    wantf = e.facets_of_all_documents()
    assert wantf == m.all_facets()
    browsed = 0
    for r in range(2):
        res, allf = got[r]
        assert allf == wantf, r
        for q, a, w in zip(qs, res, want):
            assert_same(a, w, (r, q.text, q.filter))
            if not q.text.strip() and q.enable_facets:
                m.check(a, q.filter, q.max_number_of_records_to_return, (r, q.filter)); browsed += 1
    assert browsed >= 2 * 19
