"""What Query.collapse_by costs: 1000-query batches, top-20, CoverageDepth 500, on one session.

    python tools/bench_collapse.py [--docs 10000000] [--steps 10] [--warmup 3] [--batch 1000] [--plain-only]

An index of `docs` synthetic documents (config 5) carries three columns of 10, 4096 and `docs` distinct values.  The same batches run plain (share 0 %: no
option installed, the path of every batch before the option existed) and with collapse_by on 10 % and on 100 % of their queries, keep 1 and 3, on each of the
three columns.  Per case: the median wall time of a batch (search_packed, options installed just before it), and the medians of k_finalize's and k_collapse's
durations from Session.last_timings(kernels=True) — HIP events on the session's stream; with a collapsing query k_finalize is the windowed launch, which
writes `depth` rows for those queries.  --plain-only runs the plain case alone and touches nothing of the option: it runs on a build without it, for the
comparison of the 0 % row.  Prints one JSON line per case; needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infidex_amd import SearchEngine, Query  # noqa: E402
from infidex_amd.engine import Session, pack_texts  # noqa: E402
from tools.synth import Synth  # noqa: E402

K, DEPTH = 20, 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    syn = Synth(5, docs=a.docs)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, syn.field_weights)
    rng = np.random.default_rng(17)
    if not a.plain_only:
        e.set_column("c10", rng.integers(0, 10, a.docs).astype(np.int64), facetable=False)
        e.set_column("c4096", rng.integers(0, 4096, a.docs).astype(np.int64), facetable=False)
        e.set_column("cuniq", rng.permutation(a.docs).astype(np.int64), facetable=False)
    n = a.warmup + a.steps
    qa, qo = syn.queries(n * a.batch, qseed=1000)
    texts = Synth.texts(qa, qo)
    tb = [texts[i * a.batch:(i + 1) * a.batch] for i in range(n)]
    packed = [pack_texts(t) for t in tb]
    se = Session(e)

    def run(case, install):
        wall, fin, clp, rows = [], [], [], 0
        for i in range(n):
            t0 = time.perf_counter()
            if install is not None:
                install(i)
            counts = se.search_packed(*packed[i], K, DEPTH, True)[3]
            dt = (time.perf_counter() - t0) * 1e3
            if i < a.warmup:
                continue
            t = se.last_timings(kernels=True)
            wall.append(dt); fin.append(t.get("k_finalize_rows_ms") or t["k_finalize_ms"]); clp.append(t.get("k_collapse_ms", 0.0)); rows += int(counts.sum())
        case.update({"docs": a.docs, "batch": a.batch, "steps": a.steps, "batch_ms_median": round(float(np.median(wall)), 3), "batch_ms_min": round(min(wall), 3),
                     "batch_ms_max": round(max(wall), 3), "k_finalize_ms_median": round(float(np.median(fin)), 4), "k_collapse_ms_median": round(float(np.median(clp)), 4),
                     "rows_per_query": round(rows / (a.steps * a.batch), 2)})
        print(json.dumps(case), flush=True)
    run({"case": "plain", "share": 0.0}, None)
    if a.plain_only:
        return
    from infidex_amd.engine import _install_collapse
    for share in (0.1, 1.0):
        for keep in (1, 3):
            for col in ("c10", "c4096", "cuniq"):
                pick = np.random.default_rng(5).random(a.batch) < share
                qs = [Query("", K, DEPTH, collapse_by=col if pick[j] else None, collapse_keep=keep) for j in range(a.batch)]
                run({"case": "collapse", "share": share, "keep": keep, "column": col, "collapsing_queries": int(pick.sum())}, lambda i: _install_collapse(e, se.h, qs))
                assert se.last_collapse_stats() == (int(pick.sum()), 1)
    run({"case": "plain again", "share": 0.0}, None)
    assert se.last_collapse_stats() == (0, 0)


if __name__ == "__main__":
    main()
