"""bucket_stats across two real ranks (two processes, torch.distributed gloo, both on GPU 0): every rank holds the whole columns and the global Deleted flags,
so each adds over the whole corpus on its own GPU — ShardedSearcher.bucket_stats needs no collective and must return, on every rank, the same repr as the
unsharded engine for the same requests, before and after a deletion.  70 000 documents: rank 0 owns the first 65 536, rank 1 the rest."""
import math
import os
import pickle
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

D = 70000
GONE = sorted(set(range(0, D, 7)) | {D - 1})


def requests():
    from infidex_amd import BucketStatsRequest as B
    return [B("year >= 2000 AND rating > 7.0", "rating", "year", (2000, 2005, 2010, 2015, 2020, 2025)), B("block >= 16", "block", "block", (0, 16, 17, 18)),
            B(None, "year", "rating", (float("-inf"), 0.0, 2.5, 5.0, 7.5, float("inf"))), B(None, "rating", "block", tuple(range(0, 257)))]


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
from tests.test_gpu_bucket_stats_ranks import engine_columns, requests, D, GONE
from tools.synth import Synth
s = Synth(2, docs=D); arena, offs = s.docs()
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights)
engine_columns(eng)
ss = ShardedSearcher(eng, TorchComm(dist))
live = ss.bucket_stats(requests())
stats = [ss.last_bucket_stats_stats()]
r = requests()[1]
one = ss.bucket_stats(r.filter, r.field, r.bucket_by, r.edges)
stats.append(ss.last_bucket_stats_stats())
eng.delete_documents(GONE)
dead = ss.bucket_stats(requests())
stats.append(ss.last_bucket_stats_stats())
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump((repr(live), repr(one), repr(dead), stats), f)
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
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29665", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s = Synth(2, docs=D); arena, offs = s.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights)
    engine_columns(e)
    reqs = requests()
    want_live = e.bucket_stats(reqs)
    e.delete_documents(GONE)
    want_dead = e.bucket_stats(reqs)
    for w in want_live + want_dead:
        assert w.error is None and w.nan.size + w.below.size + sum(b.size for b in w.buckets) + w.above.size == w.total == w.whole.size
    # the unsharded engine itself against the columns' values
    year, rating, _ = columns(D)
    year = np.asarray(year, np.int64); r = np.asarray(rating, np.float64)
    a = want_live[2]                                              # year per rating band
    assert a.total == D and a.whole.sum == int(year.sum()) and a.nan.size == int(np.isnan(r).sum()) and a.nan.sum == int(year[np.isnan(r)].sum())
    with np.errstate(invalid="ignore"):
        assert [b.sum for b in a.buckets] == [int(year[(r >= lo) & (r < up)].sum()) for lo, up in zip(reqs[2].edges, reqs[2].edges[1:])] and a.below.size == a.above.size == 0
    b = want_live[3]                                              # rating per block of 4096 documents: buckets are runs of consecutive documents
    assert [x.size for x in b.buckets[:18]] == [4096] * 17 + [D - 17 * 4096] and all(x.size == 0 for x in b.buckets[18:])
    assert [x.sum for x in b.buckets[:18]] == [math.fsum(v[np.isfinite(v)]) for v in (r[k * 4096:(k + 1) * 4096] for k in range(18))]
    c = want_live[1]                                              # rank 1's side of the corpus
    assert c.total == D - 65536 and [x.size for x in c.buckets] == [0, 4096, D - 65536 - 4096] and c.buckets[1].sum == 16 * 4096 and c.buckets[2].min == c.buckets[2].max == 17
    assert want_dead[1].total < c.total and want_dead[2].total == D - len(GONE)
    for rk in range(2):
        live, one, dead, stats = got[rk]
        assert live == repr(want_live) and dead == repr(want_dead), rk
        assert one == repr(want_live[1])
        assert stats == [(2, 0, 1), (0, 1, 1), (2, 0, 1)], (rk, stats)
