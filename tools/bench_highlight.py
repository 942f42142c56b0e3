"""What Query.highlight costs: 1000-query batches, top-20, CoverageDepth 500, on one session.

    python tools/bench_highlight.py [--config 4] [--docs 0] [--rounds 5] [--steps 8] [--warmup 3] [--batch 1000] [--chars 160] [--plain-only]

An index of synthetic documents in the benchmark's corpus shape (tools/synth.py; --docs 0 = the config's full size).  The same batches run plain (no option
installed: the path of every batch before the option existed) and with highlight on every query, INTERLEAVED: `rounds` times a leg of `steps` plain batches,
then a leg of `steps` highlighted ones.  Per leg: queries/s over the leg's wall time, the median of k_stage2's duration (Session.last_timings(kernels=True):
HIP events on the session's stream), and for the highlighted legs the median of k_highlight's duration, the bytes of rows a batch downloads and the rows per
query.  --plain-only runs the plain legs alone and touches nothing of the option: it runs on a build without it, for the comparison against the parent
commit.  Prints one JSON line per leg and one summary line per case (median and spread over the rounds); needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infidex_amd import SearchEngine  # noqa: E402
from infidex_amd.engine import Session, pack_texts  # noqa: E402
from tools.synth import Synth  # noqa: E402

K, DEPTH = 20, 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--docs", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--chars", type=int, default=160)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    syn = Synth(a.config, docs=a.docs or None)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0); e.index_flat(None, arena, offs, syn.field_weights)
    nb = a.warmup + a.steps
    qa, qo = syn.queries(nb * a.batch, qseed=1000)
    texts = Synth.texts(qa, qo)
    packed = [pack_texts(texts[i * a.batch:(i + 1) * a.batch]) for i in range(nb)]
    se = Session(e)
    chars = np.full(a.batch, a.chars, np.int32)

    def install():
        import ctypes as C
        e._check(e.L.infx_engine_set_query_highlight(se.h, a.batch, chars.ctypes.data_as(C.POINTER(C.c_int32)), None))

    def leg(case, lit, round_):
        s2, hl, nbytes, rows, wall = [], [], 0, 0, 0.0
        for i in range(nb):
            t0 = time.perf_counter()
            if lit:
                install()
            counts = se.search_packed(*packed[i], K, DEPTH, True)[3]
            dt = time.perf_counter() - t0
            if i < a.warmup and round_ == 0:
                continue
            wall += dt; rows += int(counts.sum())
            s2.append(se.last_timings(kernels=True)["k_stage2_ms"])
            if lit:
                ms, nbytes = se.last_highlight_timings(); hl.append(ms)
                assert se.last_highlight_stats() == (a.batch, 1)
            elif not a.plain_only:
                assert se.last_highlight_stats() == (0, 0)
        n = len(s2)
        out = {"case": case, "tag": a.tag, "round": round_, "batches": n, "queries_per_s": round(n * a.batch / wall, 1), "k_stage2_ms_median": round(float(np.median(s2)), 4),
               "rows_per_query": round(rows / (n * a.batch), 2)}
        if lit:
            out.update({"k_highlight_ms_median": round(float(np.median(hl)), 4), "download_bytes_per_batch": int(nbytes), "bytes_per_row": int(nbytes) // (a.batch * K)})
        print(json.dumps(out), flush=True)
        return out

    legs = {"plain": [], "highlight": []}
    for r in range(a.rounds):
        legs["plain"].append(leg("plain", False, r))
        if not a.plain_only:
            legs["highlight"].append(leg("highlight", True, r))
    for case, ls in legs.items():
        if not ls:
            continue
        summary = {"summary": case, "tag": a.tag, "config": a.config, "docs": a.docs, "batch": a.batch, "rounds": len(ls)}
        for key in ("queries_per_s", "k_stage2_ms_median", "k_highlight_ms_median"):
            v = [x[key] for x in ls if key in x]
            if v:
                summary[key] = {"median": round(float(np.median(v)), 4), "min": min(v), "max": max(v)}
        for key in ("download_bytes_per_batch", "bytes_per_row", "rows_per_query"):
            if key in ls[-1]:
                summary[key] = ls[-1][key]
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
