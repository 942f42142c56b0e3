"""The calls and launches behind profiles/field_stats.md: field_stats at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus three
random int group columns of 8, 100 and 4000 values (`g8`, `g100`, `g4000`).  Two runs, because a kernel trace slows the host:

    python tools/bench_field_stats.py --out calls.json                                      # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_field_stats.py
    python tools/bench_field_stats.py --summarize trace/<host>/<pid>_kernel_trace.csv [calls.json]

Cases: the statistics of `rating` (a double column, two limbs) ungrouped and grouped by g8, g100 and g4000 (its slots are in global memory), each under
`rating >= 1.0` (every document), `year >= 2000 AND rating > 7.0` (11 %) and `year = 1987 AND rating >= 1.0` (1.3 %); three requests sharing the 11 %
filter (rating ungrouped, rating by g8, year by g100); sixteen requests over four filters (the three and `year < 1990`): rating ungrouped, rating by g100,
year by g8, year by g4000.

The yardstick of a case is k_range_counts with 8 buckets over the same masks and value columns, one range request per field_stats request, in ONE launch
of the same trace: before every field_stats call the tool asks range_facets for the same (filter, field) pairs.  field_stats is not compared with itself.

Every repetition starts a new mask epoch (restore_documents), asks the ranges (which builds the masks), then asks the statistics twice, timing the second
call ("masks cached").  With --out a second loop times the first field_stats call of a new epoch, which builds its masks in front ("new epoch"; the
profiler-off run only, so the traced run's launch sequence stays fixed).  The first repetition of a case is left out; medians.  COST_DOCS overrides the
corpus size."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 4
ALL, TWO, ONE, OLD = "rating >= 1.0", "year >= 2000 AND rating > 7.0", "year = 1987 AND rating >= 1.0", "year < 1990"
VALUE_FIELDS = ["rating", "year"]
KERNELS = ("k_range_counts", "k_field_stats")


def columns():
    from tools.synth import config5_columns
    year, rating, genre = config5_columns(DOCS)
    rng = np.random.default_rng(7)
    return year, rating, genre, {"g8": rng.integers(0, 8, DOCS).astype(np.int64), "g100": rng.integers(0, 100, DOCS).astype(np.int64), "g4000": rng.integers(0, 4000, DOCS).astype(np.int64)}


def edges_of(year, rating):
    y = tuple(sorted(set(int(v) for v in np.linspace(int(year.min()), int(year.max()) + 1, 9))))
    r = tuple(float(v) for v in np.linspace(float(np.nanmin(rating)), float(np.nanmax(rating)) + 0.01, 9))
    return {"year": y, "rating": r}


def cases():
    """name -> [(filter, field, group_by)]"""
    out = {}
    for g in (None, "g8", "g100", "g4000"):
        for fname, x in (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE)):
            out["rating, %s, %s" % ("ungrouped" if g is None else "by " + g, fname)] = [(x, "rating", g)]
    out["three requests, one filter (11 %)"] = [(TWO, "rating", None), (TWO, "rating", "g8"), (TWO, "year", "g100")]
    out["sixteen requests, four filters"] = [(x, f, g) for x in (ALL, TWO, ONE, OLD) for f, g in (("rating", None), ("rating", "g100"), ("year", "g8"), ("year", "g4000"))]
    return out


def sequence():
    """The traced kernels in launch order: (case, rep, kernel)."""
    out = []
    for _ in VALUE_FIELDS:                                             # the calls that build the sort ranks and the value tables
        out += [(None, 0, "k_range_counts"), (None, 0, "k_field_stats")]
    for name in cases():
        for rep in range(REPS):
            out += [(name, rep, "k_range_counts"), (name, rep, "k_field_stats"), (name, rep, "k_field_stats")]
    return out


def summarize(path, calls_path=None):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    seq = sequence()
    assert [k for _, k, _ in rows] == [s[2] for s in seq], "the trace does not hold the launches of one run of this tool (%d launches, %d expected)" % (len(rows), len(seq))
    sts, rng = {}, {}
    for (name, rep, kern), (_, _, d) in zip(seq, rows):
        if rep:
            (sts if kern == "k_field_stats" else rng).setdefault(name, []).append(d)
    calls = json.load(open(calls_path)) if calls_path else {}
    print("| case | requests | k_field_stats (us) | k_range_counts, 8 buckets, same requests (us) | k_field_stats / k_range_counts | call, masks cached (ms) | call, new epoch (ms) |")
    print("|" + "---|" * 7)
    for name, reqs in cases().items():
        k, y = float(np.median(sts[name])), float(np.median(rng[name]))
        cc = calls.get(name, {})
        print("| %s | %d | %.1f | %.1f | %.2f | %s | %s |" % (name, len(reqs), k, y, k / y, "%.3f" % cc["cached"] if cc else "-", "%.3f" % cc["cold"] if "cold" in cc else "-"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine, RangeRequest, StatsRequest
    from tools.synth import Synth
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre, groups = columns()
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    for g, v in groups.items():
        e.set_column(g, v, facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    E = edges_of(year, rating)
    for f in VALUE_FIELDS:                                             # the sort rank and the value table are built on first use: outside the timed calls
        t = time.perf_counter()
        e.range_facets(None, f, E[f])
        a = e.field_stats(None, f)
        print("first use of %s: %.1f ms; sum %r mean %r" % (f, (time.perf_counter() - t) * 1e3, a.sum, a.mean), flush=True)
    calls = {}
    for name, reqs in cases().items():
        sr = [StatsRequest(x, f, g) for x, f, g in reqs]
        rr = [RangeRequest(x, f, E[f]) for x, f, g in reqs]
        cached = []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch
            y = e.range_facets(rr)                                     # the yardstick's launch; builds the masks
            a = e.field_stats(sr)
            assert e.last_field_stats_stats() == (0, len({r.filter for r in sr}), 1)
            t = time.perf_counter(); b = e.field_stats(sr); cached.append(time.perf_counter() - t)
            assert repr(a) == repr(b) and all(s.error is None and s.count + s.nan == s.total == q.total for s, q in zip(a, y))
            assert all(s.min == q.min and s.max == q.max and s.nan == q.nan for s, q in zip(a, y))
        calls[name] = {"cached": float(np.median(cached[1:])) * 1e3, "totals": sorted({s.total for s in a})}
        print("PHASE %s: %d requests, totals %s, cached %.3f ms" % (name, len(sr), calls[name]["totals"], calls[name]["cached"]), flush=True)
    if out_path:                                                       # profiler-off run only: the first call of an epoch builds its masks in front
        for name, reqs in cases().items():
            sr = [StatsRequest(x, f, g) for x, f, g in reqs]
            cold = []
            for rep in range(REPS):
                e.restore_documents()
                t = time.perf_counter(); e.field_stats(sr); cold.append(time.perf_counter() - t)
                assert e.last_field_stats_stats() == (len({r.filter for r in sr}), 0, 1)
            calls[name]["cold"] = float(np.median(cold[1:])) * 1e3
            print("PHASE %s: cold %.3f ms" % (name, calls[name]["cold"]), flush=True)
        # the exactness, once, against the columns' values (the whole corpus and the 1.3 % filter)
        import math
        fin = rating[np.isfinite(rating)]
        whole = e.field_stats(None, "rating")
        assert whole.sum == math.fsum(fin) and e.field_stats(None, "year").sum == int(year.sum()), (whole.sum, math.fsum(fin))
        sel = (year == 1987) & (rating >= 1.0)
        assert e.field_stats(ONE, "rating").sum == math.fsum(rating[sel])
        print("exact sums equal math.fsum and the integer sum", flush=True)
        json.dump(calls, open(out_path, "w"), indent=1)
