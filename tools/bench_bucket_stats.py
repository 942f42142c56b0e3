"""The calls and launches behind profiles/bucket_stats.md: bucket_stats at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus two
bucket columns of 1024 values — `day`, time-like: the document's number scaled to 0 .. 1023 with a jitter of a few days, so neighbours in the corpus share a
bucket — and `mix`, the same values shuffled; and three random int group columns of 8, 12 and 256 values for the yardstick.  Two runs, because a kernel trace
slows the host:

    python tools/bench_bucket_stats.py --out calls.json                                      # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_bucket_stats.py
    python tools/bench_bucket_stats.py --summarize trace/<host>/<pid>_kernel_trace.csv [calls.json]

Cases: `rating` (a double column, two limbs) in 8, 12 and 256 equal buckets of `day` and of `mix`, each under `rating >= 1.0` (every document),
`year >= 2000 AND rating > 7.0` (11 %) and `year = 1987 AND rating >= 1.0` (1.3 %); `year` (an int column, one limb) in 12 buckets of both columns over every
document; three requests sharing the 11 % filter (rating by day in 12, year by day in 12, rating by mix in 8); sixteen requests over four filters (the three
and `year < 1990`): rating by day in 12, rating by mix in 256, year by day in 8, year by mix in 12.

The yardsticks of a case come from the same trace, one launch each, and never from k_bucket_stats itself: k_range_counts with the same (filter, bucket
column, edges), one range request per bucket_stats request, and k_field_stats over the same (filter, field) grouped by a random column of as many values as
the request has buckets (g8, g12, g256).  With --out a second loop times what the call replaces for the 8- and 12-bucket cases: the B + 3 separate field_stats
calls (the whole, below, the B buckets, above) with composed filters, masks cached.

Every repetition starts a new mask epoch (restore_documents), asks the yardsticks (which builds the masks), then asks bucket_stats twice, timing the second
call ("masks cached").  The first repetition of a case is left out; medians.  COST_DOCS overrides the corpus size; INFX_LIB selects a variant of the library
(infidex_amd/build.py --variant=plain:-DBKS_MERGE_RUNS=0, the form without run merging)."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 4
DAYS = 1024
ALL, TWO, ONE, OLD = "rating >= 1.0", "year >= 2000 AND rating > 7.0", "year = 1987 AND rating >= 1.0", "year < 1990"
PCT = (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE))
VALUE_FIELDS = ["rating", "year"]
KERNELS = ("k_range_counts", "k_field_stats", "k_bucket_stats")


def columns():
    from tools.synth import config5_columns
    year, rating, genre = config5_columns(DOCS)
    rng = np.random.default_rng(7)
    day = np.clip(np.arange(DOCS, dtype=np.int64) * DAYS // DOCS + rng.integers(-3, 4, DOCS), 0, DAYS - 1).astype(np.int64)
    extra = {"day": day, "mix": rng.permutation(day)}
    for g in (8, 12, 256):
        extra["g%d" % g] = rng.integers(0, g, DOCS).astype(np.int64)
    return year, rating, genre, extra


def edges(b):
    return tuple(int(v) for v in np.linspace(0, DAYS, b + 1))


def cases():
    """name -> [(filter, field, bucket_by, buckets)]"""
    out = {}
    for by in ("day", "mix"):
        for b in (8, 12, 256):
            for fname, x in PCT:
                out["rating by %s, %d buckets, %s" % (by, b, fname)] = [(x, "rating", by, b)]
    for by in ("day", "mix"):
        out["year by %s, 12 buckets, 100 %%" % by] = [(ALL, "year", by, 12)]
    out["three requests, one filter (11 %)"] = [(TWO, "rating", "day", 12), (TWO, "year", "day", 12), (TWO, "rating", "mix", 8)]
    out["sixteen requests, four filters"] = [(x, f, by, b) for x in (ALL, TWO, ONE, OLD) for f, by, b in (("rating", "day", 12), ("rating", "mix", 256), ("year", "day", 8), ("year", "mix", 12))]
    return out


def sequence():
    """The traced kernels in launch order: (case, rep, kernel)."""
    out = []
    for _ in VALUE_FIELDS:                                             # the calls that build the sort ranks and the value tables
        for _ in ("day", "mix"):
            out += [(None, 0, "k_range_counts"), (None, 0, "k_field_stats"), (None, 0, "k_bucket_stats")]
    for name in cases():
        for rep in range(REPS):
            out += [(name, rep, "k_range_counts"), (name, rep, "k_field_stats"), (name, rep, "k_bucket_stats"), (name, rep, "k_bucket_stats")]
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
    rows = rows[:len(seq)]                                             # (an --out run's replaced calls follow the sequence)
    assert [k for _, k, _ in rows] == [s[2] for s in seq], "the trace does not hold the launches of one run of this tool (%d launches, %d expected)" % (len(rows), len(seq))
    t = {k: {} for k in KERNELS}
    for (name, rep, kern), (_, _, d) in zip(seq, rows):
        if rep:
            t[kern].setdefault(name, []).append(d)
    calls = json.load(open(calls_path)) if calls_path else {}
    print("| case | requests | k_bucket_stats (us) | k_field_stats, grouped by as many values (us) | k_range_counts, same edges (us) | / k_field_stats | / k_range_counts | call, masks cached (ms) | the B + 3 field_stats calls it replaces (ms) |")
    print("|" + "---|" * 9)
    for name, reqs in cases().items():
        k, s, y = (float(np.median(t[kern][name])) for kern in ("k_bucket_stats", "k_field_stats", "k_range_counts"))
        cc = calls.get(name, {})
        print("| %s | %d | %.1f | %.1f | %.1f | %.2f | %.2f | %s | %s |" % (name, len(reqs), k, s, y, k / s, k / y, "%.3f" % cc["cached"] if cc else "-", "%.3f" % cc["replaced"] if "replaced" in cc else "-"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine, RangeRequest, StatsRequest, BucketStatsRequest
    from tools.synth import Synth
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre, extra = columns()
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    for g, v in extra.items():
        e.set_column(g, v, facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    for f in VALUE_FIELDS:                                             # the sort ranks and the value table are built on first use: outside the timed calls
        for by in ("day", "mix"):
            t = time.perf_counter()
            e.range_facets(None, by, edges(8)); e.field_stats(None, f, "g8")
            a = e.bucket_stats(None, f, by, edges(8))
            print("first use of %s by %s: %.1f ms; whole sum %r" % (f, by, (time.perf_counter() - t) * 1e3, a.whole.sum), flush=True)
    calls = {}
    for name, reqs in cases().items():
        br = [BucketStatsRequest(x, f, by, edges(b)) for x, f, by, b in reqs]
        rr = [RangeRequest(x, by, edges(b)) for x, f, by, b in reqs]
        sr = [StatsRequest(x, f, "g%d" % b) for x, f, by, b in reqs]
        cached = []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch
            y = e.range_facets(rr)                                     # the yardsticks' launches; the first builds the masks
            s = e.field_stats(sr)
            a = e.bucket_stats(br)
            assert e.last_bucket_stats_stats() == (0, len({r.filter for r in br}), 1)
            t = time.perf_counter(); b2 = e.bucket_stats(br); cached.append(time.perf_counter() - t)
            assert repr(a) == repr(b2) and all(x.error is None and [r.size for r in x.buckets] == q.counts and x.total == q.total for x, q in zip(a, y))
            assert all(repr((x.whole.count, x.whole.nan, x.whole.min, x.whole.max, x.whole.sum, x.whole.mean)) == repr((q.count, q.nan, q.min, q.max, q.sum, q.mean)) for x, q in zip(a, s))
        calls[name] = {"cached": float(np.median(cached[1:])) * 1e3, "totals": sorted({x.total for x in a}), "place": list(e.last_bucket_stats_placement())}
        print("PHASE %s: %d requests, totals %s, place %s, cached %.3f ms" % (name, len(br), calls[name]["totals"], calls[name]["place"], calls[name]["cached"]), flush=True)
    if out_path:                                                       # profiler-off run only: what a chart of 8 or 12 buckets cost before, B + 3 calls with composed filters
        for name, reqs in cases().items():
            if len(reqs) != 1 or reqs[0][3] > 12:
                continue
            x, f, by, b = reqs[0]
            ed = edges(b)
            exprs = [x, "%s AND %s < %d" % (x, by, ed[0])] + ["%s AND %s >= %d AND %s < %d" % (x, by, lo, by, up) for lo, up in zip(ed, ed[1:])] + ["%s AND %s >= %d" % (x, by, ed[-1])]
            assert len(exprs) == b + 3
            took = []
            for rep in range(REPS):
                if rep == 0:
                    e.restore_documents()
                t = time.perf_counter()
                parts = [e.field_stats(z, f) for z in exprs]
                took.append(time.perf_counter() - t)
            a = e.bucket_stats(x, f, by, ed)
            assert [p.total for p in parts[1:]] == [a.below.size] + [r.size for r in a.buckets] + [a.above.size] and [repr(p.sum) for p in parts[2:-1]] == [repr(r.sum) for r in a.buckets]
            calls[name]["replaced"] = float(np.median(took[1:])) * 1e3
            print("PHASE %s: the %d calls it replaces %.3f ms" % (name, b + 3, calls[name]["replaced"]), flush=True)
        json.dump(calls, open(out_path, "w"), indent=1)
