"""The calls and launches behind profiles/field_quantiles.md: field_quantiles at 10 M documents on the corpus of tools/bench_field_stats.py (config-5 columns:
year 75 values, rating 91) plus three random int group columns of 7, 1000 and 4096 values (`q7`, `q1000`, `q4096`) and `wide`, an int column of about a
million values (20 bits of keys: two passes at 11-bit digits).  Two runs, because a kernel trace slows the host:

    python tools/bench_field_quantiles.py --out calls.json                                  # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_field_quantiles.py --plan plan.json
    python tools/bench_field_quantiles.py --summarize trace/<host>/<pid>_kernel_trace.csv plan.json [calls.json]

Cases: 1, 5 and 16 quantiles of `rating`, ungrouped, under `rating >= 1.0` (every document), `year >= 2000 AND rating > 7.0` (11 %) and
`year = 1987 AND rating >= 1.0` (1.3 %); 5 quantiles by q7, q1000 and q4096 at 100 % and 11 %; the median of `wide` at 100 % and 11 %; sixteen requests
over four filters (the three and `year < 1990`): rating 5 quantiles ungrouped, rating the median by q7, year 16 quantiles ungrouped, wide 5 quantiles by q1000.

The yardstick of a case with ONE ungrouped request is the way to its first figure before field_quantiles existed:
list_documents(filter, order_by=field, offset=nan + floor((count - 1) * q), limit=1), asked in the same run right behind it and checked to list a document
of the same value.

Every repetition starts a new mask epoch (restore_documents), asks once (which builds the masks), then times the second call ("masks cached").  The first
repetition of a case is left out; medians.  --plan records, per timed call, how many launches it made, for --summarize to cut the trace by.  COST_DOCS
overrides the corpus size."""
import csv
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 4
ALL, TWO, ONE, OLD = "rating >= 1.0", "year >= 2000 AND rating > 7.0", "year = 1987 AND rating >= 1.0", "year < 1990"
Q1, Q5 = (0.5,), (0.0, 0.25, 0.5, 0.75, 1.0)
Q16 = tuple(i / 15 for i in range(16))
QUANT_KERNELS, LIST_KERNELS = ("k_quant_hist", "k_quant_pick"), ("k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort")


def columns():
    from tools.synth import config5_columns
    year, rating, genre = config5_columns(DOCS)
    rng = np.random.default_rng(17)
    extra = {"q7": rng.integers(0, 7, DOCS).astype(np.int64), "q1000": rng.integers(0, 1000, DOCS).astype(np.int64), "q4096": rng.integers(0, 4096, DOCS).astype(np.int64),
             "wide": rng.integers(0, 1 << 20, DOCS).astype(np.int64) * 5 - 77}
    return year, rating, genre, extra


def cases():
    """name -> [(filter, field, q, group_by)]"""
    out = {}
    for qn, q in (("1 quantile", Q1), ("5 quantiles", Q5), ("16 quantiles", Q16)):
        for fname, x in (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE)):
            out["rating, %s, ungrouped, %s" % (qn, fname)] = [(x, "rating", q, None)]
    for g in ("q7", "q1000", "q4096"):
        for fname, x in (("100 %", ALL), ("11 %", TWO)):
            out["rating, 5 quantiles, by %s, %s" % (g, fname)] = [(x, "rating", Q5, g)]
    for fname, x in (("100 %", ALL), ("11 %", TWO)):
        out["wide, 1 quantile, ungrouped, %s" % fname] = [(x, "wide", Q1, None)]
    out["sixteen requests, four filters"] = [(x, f, q, g) for x in (ALL, TWO, ONE, OLD) for f, q, g in (("rating", Q5, None), ("rating", Q1, "q7"), ("year", Q16, None), ("wide", Q5, "q1000"))]
    return out


def has_yardstick(reqs):
    return len(reqs) == 1 and reqs[0][3] is None


def summarize(path, plan_path, calls_path=None):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in QUANT_KERNELS + LIST_KERNELS:
                if k in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    plan = json.load(open(plan_path))
    assert sum(p["launches"] for p in plan) == len(rows), "the trace does not hold the launches of one run of this tool (%d launches, %d expected)" % (len(rows), sum(p["launches"] for p in plan))
    at = 0; quant, lst = {}, {}
    for p in plan:
        part = rows[at:at + p["launches"]]; at += p["launches"]
        assert all(k in (QUANT_KERNELS if p["kind"] == "quant" else LIST_KERNELS) for _, k, _ in part), (p, [k for _, k, _ in part])
        if p["timed"]:
            (quant if p["kind"] == "quant" else lst).setdefault(p["case"], []).append(sum(d for _, _, d in part))
    calls = json.load(open(calls_path)) if calls_path else {}
    print("| case | requests | digit bits | passes | (request, pass) bins in LDS / global | kernels (us) | call (ms) | list_documents kernels (us) | list_documents call (ms) | kernels / list_documents |")
    print("|" + "---|" * 10)
    for name, reqs in cases().items():
        k = float(np.median(quant[name])); cc = calls.get(name, {})
        y = float(np.median(lst[name])) if name in lst else None
        print("| %s | %d | %s | %s | %s | %.1f | %s | %s | %s | %s |" % (
            name, len(reqs), cc.get("bits", "-"), cc.get("passes", "-"), "%d / %d" % tuple(cc["placed"]) if cc else "-", k, "%.3f" % cc["cached"] if cc else "-",
            "%.1f" % y if y is not None else "-", "%.3f" % cc["list"] if "list" in cc else "-", "%.2f" % (k / y) if y is not None else "-"))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    plan_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--plan" else None
    from infidex_amd import SearchEngine, QuantileRequest
    from tools.synth import Synth
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre, extra = columns()
    cols = dict(extra, year=year, rating=rating)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    for g, v in extra.items():
        e.set_column(g, v, facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    plan = []

    def note(case, kind, timed):
        # the traced launches of the call: its histogram and pick launches, or the listing's kernels; a mask build in front is not among the traced names
        st = e.last_field_quantiles_stats() if kind == "quant" else e.last_list_stats()
        launches = 2 * st[2] if kind == "quant" else st[3] - (1 if st[0] else 0)
        plan.append({"case": case, "kind": kind, "timed": timed, "launches": int(launches)})

    for f in ("rating", "year", "wide"):                               # the sort rank is built on first use: outside the timed calls
        t = time.perf_counter()
        a = e.field_quantiles(None, f, Q5); note(None, "quant", False)
        print("first use of %s: %.1f ms; %r" % (f, (time.perf_counter() - t) * 1e3, a.values), flush=True)
    calls = {}
    for name, reqs in cases().items():
        qr = [QuantileRequest(x, f, q, g) for x, f, q, g in reqs]
        cached, listed = [], []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch
            a = e.field_quantiles(qr); note(name, "quant", False)      # builds the masks
            t = time.perf_counter(); b = e.field_quantiles(qr); cached.append(time.perf_counter() - t); note(name, "quant", rep > 0)
            assert e.last_field_quantiles_stats()[:2] == (0, len({r.filter for r in qr}))
            assert repr(a) == repr(b) and all(s.error is None and s.count + s.nan == s.total for s in a)
            if has_yardstick(reqs):                                    # the parent's way to the first figure
                x, f, q, _ = reqs[0]
                off = a[0].nan + math.floor((a[0].count - 1) * q[0])
                t = time.perf_counter(); page = e.list_documents(x, f, True, off, 1); listed.append(time.perf_counter() - t); note(name, "list", rep > 0)
                assert e.last_list_stats()[:2] == (0, 1) and cols[f][page.document_ids[0]] == a[0].values[0], (name, page, a[0].values[0])
        bits, lds, glob = e.last_field_quantiles_placement()
        calls[name] = {"cached": float(np.median(cached[1:])) * 1e3, "totals": sorted({s.total for s in a}), "bits": bits, "passes": e.last_field_quantiles_stats()[2], "placed": [lds, glob]}
        if listed:
            calls[name]["list"] = float(np.median(listed[1:])) * 1e3
        print("PHASE %s: %d requests, totals %s, bits %d, passes %d, LDS / global %d / %d, cached %.3f ms%s" % (
            name, len(qr), calls[name]["totals"], bits, calls[name]["passes"], lds, glob, calls[name]["cached"], ", list_documents %.3f ms" % calls[name]["list"] if listed else ""), flush=True)
    if plan_path:
        json.dump(plan, open(plan_path, "w"))
    if out_path:
        # the exactness, once, against the columns' values (the whole corpus and the 1.3 % filter; by q7 under the 11 % filter)
        for x, sel in ((None, np.ones(DOCS, bool)), (ONE, (year == 1987) & (rating >= 1.0))):
            for f in ("rating", "wide"):
                w = np.sort(cols[f][sel])
                assert e.field_quantiles(x, f, Q16).values == [w[math.floor((len(w) - 1) * q)].item() for q in Q16], (x, f)
        sel = (year >= 2000) & (rating > 7.0)
        by = {g.value: g.values for g in e.field_quantiles(TWO, "wide", Q5, "q7").groups}
        for v in range(7):
            w = np.sort(cols["wide"][sel & (extra["q7"] == v)])
            assert by[str(v)] == [w[math.floor((len(w) - 1) * q)].item() for q in Q5], v
        print("quantiles equal a numpy sort of the values", flush=True)
        json.dump(calls, open(out_path, "w"), indent=1)
