"""The calls and launches behind profiles/range_facets.md: range_facets at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus a
unique int column (`uid`).  Two runs, because a kernel trace slows the host:

    python tools/bench_range_facets.py --out calls.json                                     # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_range_facets.py
    python tools/bench_range_facets.py --summarize trace/<host>/<pid>_kernel_trace.csv [calls.json]

Cases: one request over `year` with 8 buckets, one over `uid` with 256 buckets and one over `uid` with 8 (the bucket count apart from the rank gather), each
under `rating >= 1.0` (every document), `year >= 2000 AND rating > 7.0` (11 %) and `year = 1987 AND rating >= 1.0` (1.3 %); three requests (year 8, rating 8,
uid 256 buckets) sharing the 11 % filter; sixteen requests over four filters (the three and `year < 1990`), four fields each.

The yardstick of a request is list_documents' k_list_hist over the same mask and column — the same walk with a histogram behind it — from the same trace:
before every range_facets call the tool lists one row per request (list_documents(filter, order_by=field, limit=1)); the FIRST histogram pass of that
listing counts every member and is the one compared (uid takes three passes).

Every repetition starts a new mask epoch (restore_documents), lists (which builds the masks), then asks the ranges twice, timing the second call ("masks
cached").  With --out a second loop times the first range call of a new epoch, which builds its masks in front ("new epoch"; the profiler-off run only, so
the traced run's launch sequence stays fixed).  The first repetition of a case is left out; medians.  COST_DOCS overrides the corpus size."""
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
FIELDS = ["year", "rating", "uid"]
KERNELS = ("k_list_hist", "k_range_counts")


def passes(nvals, bits=11):
    return ((nvals + 1).bit_length() + bits - 1) // bits


def columns():
    from tools.synth import config5_columns
    year, rating, genre = config5_columns(DOCS)
    uid = np.random.default_rng(7).permutation(np.arange(DOCS, dtype=np.int64))
    return year, rating, genre, uid


def edges_of(year, rating):
    y = tuple(sorted(set(int(v) for v in np.linspace(int(year.min()), int(year.max()) + 1, 9))))
    r = tuple(float(v) for v in np.linspace(float(np.nanmin(rating)), float(np.nanmax(rating)) + 0.01, 9))
    u8 = tuple(int(v) for v in np.linspace(0, DOCS, 9))
    u = tuple(sorted(set(int(v) for v in np.linspace(0, DOCS, 257))))
    y256 = tuple(range(int(year.min()) - 90, int(year.min()) - 90 + 257))
    return {"year8": ("year", y), "rating8": ("rating", r), "uid8": ("uid", u8), "uid256": ("uid", u), "year256": ("year", y256)}


def cases():
    """name -> [(filter, edge set name)]"""
    out = {}
    for fname, x in (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE)):
        out["year, 8 buckets, %s" % fname] = [(x, "year8")]
    for fname, x in (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE)):
        out["uid, 256 buckets, %s" % fname] = [(x, "uid256")]
    for fname, x in (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE)):
        out["uid, 8 buckets, %s" % fname] = [(x, "uid8")]
    out["three requests, one filter (11 %)"] = [(TWO, "year8"), (TWO, "rating8"), (TWO, "uid256")]
    out["sixteen requests, four filters"] = [(x, k) for x in (ALL, TWO, ONE, OLD) for k in ("year8", "rating8", "uid256", "year256")]
    return out


def sequence(nvals, E):
    """The traced kernels in launch order: (case, rep, request or None, kernel, pass)."""
    out = []
    for f in FIELDS:                                                   # the calls that build the sort ranks
        out += [(None, 0, None, "k_list_hist", p) for p in range(passes(nvals[f]))] + [(None, 0, None, "k_range_counts", 0)]
    for name, reqs in cases().items():
        for rep in range(REPS):
            for i, (x, k) in enumerate(reqs):
                out += [(name, rep, i, "k_list_hist", p) for p in range(passes(nvals[E[k][0]]))]
            out += [(name, rep, None, "k_range_counts", 0), (name, rep, None, "k_range_counts", 1)]
    return out


def summarize(path, calls_path=None):
    year, rating, genre, uid = columns()
    nvals = {"year": len(np.unique(year)), "rating": len(np.unique(rating)), "uid": DOCS}
    E = edges_of(year, rating)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    seq = sequence(nvals, E)
    assert [k for _, k, _ in rows] == [s[3] for s in seq], "the trace does not hold the launches of one run of this tool (%d launches, %d expected)" % (len(rows), len(seq))
    rng, hist = {}, {}
    for (name, rep, req, kern, p), (_, _, d) in zip(seq, rows):
        if not rep:
            continue
        if kern == "k_range_counts":
            rng.setdefault(name, []).append(d)
        elif p == 0:
            hist.setdefault(name, {}).setdefault(rep, []).append(d)
    calls = json.load(open(calls_path)) if calls_path else {}
    print("| case | requests | k_range_counts (us) | k_list_hist, first pass, one per request (us) | their sum (us) | k_range_counts / sum | call, masks cached (ms) | call, new epoch (ms) |")
    print("|" + "---|" * 8)
    for name, reqs in cases().items():
        per = [float(np.median([hist[name][rep][i] for rep in hist[name]])) for i in range(len(reqs))]
        k = float(np.median(rng[name]))
        cc = calls.get(name, {})
        print("| %s | %d | %.1f | %s | %.1f | %.2f | %s | %s |" % (name, len(reqs), k, " / ".join("%.1f" % h for h in per) if len(per) <= 4 else "%.1f .. %.1f" % (min(per), max(per)),
                                                              sum(per), k / sum(per), "%.3f" % cc["cached"] if cc else "-", "%.3f" % cc["cold"] if cc else "-"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine, RangeRequest
    from tools.synth import Synth
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre, uid = columns()
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    e.set_column("uid", uid, facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    E = edges_of(year, rating)
    for f in FIELDS:                                                   # the sort ranks and the ranks' value order are built on first use: outside the timed calls
        t = time.perf_counter()
        e.list_documents(None, f, True, 0, 1)
        e.range_facets(None, f, E[{"year": "year8", "rating": "rating8", "uid": "uid256"}[f]][1])
        print("first use of %s: %.1f ms" % (f, (time.perf_counter() - t) * 1e3), flush=True)
    calls = {}
    for name, reqs in cases().items():
        rr = [RangeRequest(x, E[k][0], E[k][1]) for x, k in reqs]
        first, cached = [], []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch
            for r in rr:
                e.list_documents(r.filter, r.field, True, 0, 1)        # the yardstick's launches; builds the masks
            t = time.perf_counter(); a = e.range_facets(rr); first.append(time.perf_counter() - t)
            assert e.last_range_stats() == (0, len({r.filter for r in rr}), 1)
            t = time.perf_counter(); b = e.range_facets(rr); cached.append(time.perf_counter() - t)
            assert a == b and all(g.error is None and g.nan + g.below + sum(g.counts) + g.above == g.total for g in a)
        calls[name] = {"cached": float(np.median(cached[1:])) * 1e3, "totals": sorted({g.total for g in a})}
        print("PHASE %s: %d requests, totals %s, cached %.3f ms" % (name, len(rr), calls[name]["totals"], calls[name]["cached"]), flush=True)
    if out_path:                                                       # profiler-off run only: the first call of an epoch builds its masks in front (no launches the trace's sequence knows)
        for name, reqs in cases().items():
            rr = [RangeRequest(x, E[k][0], E[k][1]) for x, k in reqs]
            cold = []
            for rep in range(REPS):
                e.restore_documents()
                t = time.perf_counter(); e.range_facets(rr); cold.append(time.perf_counter() - t)
                assert e.last_range_stats() == (len({r.filter for r in rr}), 0, 1)
            calls[name]["cold"] = float(np.median(cold[1:])) * 1e3
            print("PHASE %s: cold %.3f ms" % (name, calls[name]["cold"]), flush=True)
        json.dump(calls, open(out_path, "w"), indent=1)
