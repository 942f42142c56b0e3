"""CoverageSetup across two real ranks (two processes, torch.distributed gloo, both on GPU 0): the per-query batch of tests/test_gpu_coverage_setup.py through
ShardedSearcher.search_queries, and two engine-wide setups through ShardedSearcher.search_packed, must return what the unsharded engine returns."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANK_SCRIPT = r'''
import os, sys, pickle
import torch, torch.distributed as dist
torch.cuda.init()
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
from infidex_amd import CoverageSetup
from infidex_amd.engine import pack_texts
from infidex_amd.sharded import create_sharded_engine, ShardedSearcher, TorchComm
from tests import oracle_setup as S
from tests.test_gpu_coverage_setup import per_query_batch, add_columns, K
s, arena, offs = S.synth_corpus()
out = {}
eng = create_sharded_engine(rank, world, 0)
eng.index_flat(None, arena, offs, s.field_weights); add_columns(eng)
out["per_query"] = ShardedSearcher(eng, TorchComm(dist)).search_queries(per_query_batch(S.set_s2(s)))
a, off = pack_texts(S.set_s1(s))
for name, cs in (("minimal", CoverageSetup.create_minimal()), ("typos-0", CoverageSetup(num_typos=0))):
    eng = create_sharded_engine(rank, world, 0, coverage_setup=cs)
    eng.index_flat(None, arena, offs, s.field_weights)
    out[name] = ShardedSearcher(eng, TorchComm(dist)).search_packed(a, off, K)
with open(sys.argv[1] + ".%d" % rank, "wb") as f:
    pickle.dump(out, f)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_equal_unsharded(tmp_path):
    from infidex_amd import SearchEngine, CoverageSetup
    from infidex_amd.engine import pack_texts
    from tests import oracle_setup as S
    from tests.test_gpu_coverage_setup import per_query_batch, add_columns, assert_same_result, K
    out = str(tmp_path / "res")
    env = dict(os.environ); env["PYTHONPATH"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); env["INFX_THREADS"] = "4"
    script = str(tmp_path / "rank.py"); open(script, "w").write(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29647", script, out]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    got = [pickle.load(open(out + ".%d" % r, "rb")) for r in range(2)]
    s, arena, offs = S.synth_corpus()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, s.field_weights); add_columns(e)
    qs = per_query_batch(S.set_s2(s))
    want = e.search_queries(qs)
    for r in range(2):
        for q, a, w in zip(qs, got[r]["per_query"], want):
            assert_same_result(a, w, (r, q.text, q.coverage_setup))
    s1 = S.set_s1(s); a, off = pack_texts(s1)
    for name, cs in (("minimal", CoverageSetup.create_minimal()), ("typos-0", CoverageSetup(num_typos=0))):
        ref = SearchEngine.create_default(device=0, coverage_setup=cs); ref.index_flat(None, arena, offs, s.field_weights)
        rk, rs, rt, rc, rf = ref.search_packed(a, off, K)
        for r in range(2):
            k, sc, t, c, f = got[r][name]
            assert np.array_equal(c, rc) and np.array_equal(f, rf), (name, r)
            for i in range(len(s1)):
                n = int(c[i])
                assert np.array_equal(k[i, :n], rk[i, :n]) and np.array_equal(t[i, :n], rt[i, :n]) and np.array_equal(sc[i, :n].view(np.uint32), rs[i, :n].view(np.uint32)), (name, r, s1[i])
