"""`python bench.py --gpus 1` on a small corpus: a plain run prints the headline of its timed steps and runs none of the legs of `--full`; `--full` adds
them (value_long, the roofline leg, the single-query latency, the CPU baseline).  The multi-rank forms run in tests/test_gpu_sharded_ranks.py."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--docs", "100000", "--steps", "3", "--warmup", "1", "--batch", "200"]
FULL_ONLY = ("value_long", "roofline", "roofline_by_kernel", "p50_single_query_latency_ms", "cpu_baseline", "speedup_vs_cpu_baseline")


def _bench(args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "INFX_FORCE_SHARDED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(d):
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["n_gpus"] == 1
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 200 * 1000.0) < 1e-6 * 200 * 1000.0      # value = steps x batch / elapsed, ms_per_step = elapsed / steps


def test_plain_run_is_the_headline_only():
    d = _bench([])
    _check_headline(d)
    assert not [k for k in FULL_ONLY if k in d]
    assert d["p50_batch_latency_ms"] > 0 and d["stage_ms_per_step"]


def test_full_run_adds_the_other_legs():
    d = _bench(["--full", "--long-steps", "2", "--cpu-sample", "32"])
    _check_headline(d)
    assert not [k for k in FULL_ONLY if k not in d]
    assert d["value_long"]["steps"] == 2 and d["value_long"]["value"] > 0
    assert d["roofline"]["avg_launch_ms"] > 0 and d["roofline"]["achieved"] > 0 and isinstance(d["roofline_by_kernel"], list)
    assert d["p50_single_query_latency_ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["identical_topk_sets"].endswith("/32")
