"""The calls and launches behind profiles/field_distinct.md: field_distinct at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus
random int columns of 8, 100, 4000 and 100 000 values (`g8`, `g100`, `g4000`, `g100k`) and a unique one (`uid`).  One run under a kernel trace; the tool writes
what it called, in order, with every call's launch count, and the summary cuts the trace by those counts:

    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_field_distinct.py --out calls.json
    python tools/bench_field_distinct.py --summarize trace/<host>/<pid>_kernel_trace.csv calls.json > table.md

Per field — `genre` (12 values), `g100k`, `uid` — grouping — none, `g8`, `g100`, `g4000` — and filter — `rating >= 1.0` (every document),
`year >= 2000 AND rating > 7.0` (11 %), `year = 1987 AND rating >= 1.0` (1.3 %) — with the masks already in the session's cache, REPS times each:
    auto / lds / bitmap / hash   field_distinct(filter, field, group) in automatic placement and forced into each of the three; a forced placement that fell
            back to another one is left out of the table.  The walk (k_distinct_lds / _bitmap / _hash), k_distinct_count and k_distinct_union, and the memsets of the
            workspace in front of them (the trace's fill kernels between the call before and the call's last kernel)
    heads   without grouping: list_groups(filter, field, limit 1) — k_group_heads, k_group_heads_mask and the listing's select — today's way to the whole count
    mask    list_documents of the same filter under a text no cache has seen: its k_filter_mask_multi
Medians over the repetitions, the first left out.  The host times are taken under the trace, which slows the host: they are upper bounds.  COST_DOCS
overrides the corpus size."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 4
ALL, TWO, ONE = "rating >= 1.0", "year >= 2000 AND rating > 7.0", "year = 1987 AND rating >= 1.0"
FILTERS = (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE))
FIELDS = (("genre", 12), ("g100k", 100000), ("uid", 0))
GROUPS = ((None, 1), ("g8", 8), ("g100", 100), ("g4000", 4000))
MODES = (("auto", 0), ("lds", 1), ("bitmap", 2), ("hash", 3))
PLACES = ("lds", "bitmap", "hash")
KERNELS = ("k_filter_mask_multi", "k_distinct_lds", "k_distinct_bitmap", "k_distinct_hash", "k_distinct_count", "k_distinct_union", "k_group_heads_mask", "k_group_heads", "k_group_page",
           "k_group_sizes", "k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort")
WALKS = ("k_distinct_lds", "k_distinct_bitmap", "k_distinct_hash")
HEADS = ("k_group_heads", "k_group_heads_mask", "k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix")
FILL = "fill"


def kernel_of(name):
    for k in KERNELS:                                                  # (k_group_heads_mask before k_group_heads)
        if k in name:
            return k
    return FILL if "fillBuffer" in name else None


def summarize(path, calls_path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = kernel_of(r["Kernel_Name"])
            if k:
                rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    log = json.load(open(calls_path))
    need = sum(c["launches"] for c in log["calls"])
    named = [i for i, r in enumerate(rows) if r[1] != FILL]
    assert len(named) >= need, "the trace holds fewer launches (%d) than the timed calls made (%d)" % (len(named), need)
    first = named[len(named) - need]                                   # the timed calls are the last ones of the run
    while first > 0 and rows[first - 1][1] == FILL:                    # ... with the memsets in front of their first kernel
        first -= 1
    rows = rows[first:]
    by = {}
    at = 0
    for c in log["calls"]:
        d = {}; left = c["launches"]
        while left:                                                    # the call's kernels and the fills in front of each
            _, k, us = rows[at]; at += 1
            d[k] = d.get(k, 0.0) + us
            left -= k != FILL
        if c["rep"]:
            by.setdefault((c["case"], c["kind"]), []).append((d, c["ms"], c))
    med = lambda xs: float(np.median(xs)) if len(xs) else float("nan")
    print("| field | groups | filter | members | distinct | mode | placed in | walk (us) | k_distinct_count + k_distinct_union (us) | memsets (us) | kernels + memsets (us) | workspace MB "
          "| list_groups heads + select (us) | k_filter_mask_multi (us) | call (ms, under the trace) |")
    print("|" + "---|" * 15)
    masks = {}
    for (name, kind), runs in by.items():                              # the mask build depends on the filter alone
        if kind == "mask":
            masks.setdefault(name.rsplit(", ", 1)[1], []).extend(d.get("k_filter_mask_multi", 0.0) for d, _, _ in runs)
    for name in log["cases"]:
        heads = med([sum(d.get(k, 0.0) for k in HEADS) for d, _, _ in by.get((name, "heads"), [])])
        mask = med(masks.get(name.rsplit(", ", 1)[1], []))
        for mode, _ in MODES:
            runs = by.get((name, mode), [])
            if not runs:
                continue
            c = runs[0][2]
            if mode != "auto" and c["placed"] != mode:                 # forced, and fell back to a placement the case already has
                continue
            walk = med([sum(d.get(k, 0.0) for k in WALKS) for d, _, _ in runs]); cnt = med([d.get("k_distinct_count", 0.0) + d.get("k_distinct_union", 0.0) for d, _, _ in runs])
            fill = med([d.get(FILL, 0.0) for d, _, _ in runs])
            print("| %s | %s | %s | %d | %d | %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %s | %.1f | %.3f |" % (
                c["field"], c["group"] or "-", c["filter"], c["members"], c["distinct"], mode, c["placed"], walk, cnt, fill, walk + cnt + fill, c["ws_mb"],
                "%.1f" % heads if c["group"] is None else "-", mask, med([ms for _, ms, _ in runs])))


def workspace_mb(placed, G, V, docs):
    """the bytes of one spec's pair set, as the device library lays them out"""
    row = (V + 31) // 32
    if placed == "hash":
        cap = 1024
        while cap < 2 * min(docs, G * V):
            cap *= 2
        return (cap * 8 + (row * 4 if G > 1 else 0)) / 1e6
    return (G * row + (row if G > 1 else 0)) * 4 / 1e6


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine
    from tools.synth import Synth, config5_columns
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre = config5_columns(DOCS)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    rng = np.random.default_rng(7)
    cols = {"genre": np.asarray(genre)}
    for g, card in (("g8", 8), ("g100", 100), ("g4000", 4000), ("g100k", 100000), ("uid", 0)):
        cols[g] = rng.integers(0, card, DOCS).astype(np.int64) if card else rng.permutation(DOCS).astype(np.int64)
        e.set_column(g, cols[g], facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    members = {}
    for fname, x in FILTERS:                                           # warm: masks, sort ranks; the answers, once, against the columns
        members[x] = e.prefilter_mask(x) == 0
        for f, _ in FIELDS:
            e.list_groups(x, f, None, True, 0, 1)
    sel = members[ONE]
    for mode, m in MODES:
        e.set_distinct_placement(m)
        got = e.field_distinct(ONE, "g100k", "g8")
        want = [len(np.unique(cols["g100k"][sel & (cols["g8"] == v)])) for v in range(8)]
        assert sorted(g.distinct for g in got.groups) == sorted(want) and got.distinct == len(np.unique(cols["g100k"][sel])) and got.total == int(sel.sum()), (mode, got.distinct, want)
        assert e.field_distinct(TWO, "uid").distinct == int(members[TWO].sum())
    print("the counts equal numpy's on the columns in every placement", flush=True)
    log = {"cases": [], "calls": []}
    fresh = 0
    for f, fcard in FIELDS:
        for g, gcard in GROUPS:
            for fname, x in FILTERS:
                name = "%s by %s, %s" % (f, g or "-", fname)
                log["cases"].append(name)
                V = fcard or DOCS
                for rep in range(REPS):
                    def timed(kind, fn, launches):
                        t = time.perf_counter(); a = fn(); ms = (time.perf_counter() - t) * 1e3
                        rec = {"case": name, "kind": kind, "rep": rep, "ms": ms, "launches": launches()}
                        log["calls"].append(rec)
                        return a, rec
                    for mode, m in MODES:
                        e.set_distinct_placement(m)
                        a, rec = timed(mode, lambda: e.field_distinct(x, f, g), lambda: e.last_field_distinct_stats()[5])
                        st = e.last_field_distinct_stats()
                        assert st[:2] == (0, 1) and sum(st[2:5]) == 1 and a.error is None
                        placed = PLACES[st[2:5].index(1)]
                        rec.update({"field": f, "group": g, "filter": fname, "members": a.total, "distinct": a.distinct, "placed": placed, "ws_mb": workspace_mb(placed, gcard, V, DOCS)})
                    e.set_distinct_placement(0)
                    if g is None:
                        timed("heads", lambda: e.list_groups(x, f, None, True, 0, 1), lambda: e.last_group_list_stats()[4])
                        fresh += 1
                        timed("mask", lambda: e.list_documents("%s AND rating >= 0.%d" % (x, fresh), None, True, 0, 1), lambda: e.last_list_stats()[3])
                print("PHASE %s: %d members, %d distinct" % (name, a.total, a.distinct), flush=True)
    if out_path:
        json.dump(log, open(out_path, "w"), indent=1)
