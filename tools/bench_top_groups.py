"""The calls and launches behind profiles/top_groups.md: top_groups at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus random int
group columns of 8, 4000 and 100 000 values (`g8`, `g4000`, `g100k`) and a unique one (`uid`).  One run under a kernel trace; the tool writes what it called,
in order, with every call's launch count, and the summary cuts the trace by those counts:

    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_top_groups.py --out calls.json
    python tools/bench_top_groups.py --summarize trace/<host>/<pid>_kernel_trace.csv calls.json > table.md

Per group column and filter — `rating >= 1.0` (every document), `year >= 2000 AND rating > 7.0` (11 %), `year = 1987 AND rating >= 1.0` (1.3 %) — with the
masks already in the session's cache, REPS times each:
    top     top_groups(filter, g, "sum", "rating", descending, page 0 of 20): k_field_stats without a cap, k_top_keys, nine k_top_hist / k_top_pick at 11 bits
            (a double sum: 98-bit composites), k_top_gather, k_top_page
    size    top_groups(filter, g): k_top_sizes, six passes (66 bits)
    stats   field_stats(filter, "rating", g) where the column has at most 4096 values: the same accumulate kernel over the same mask and field
    heads   list_groups(filter, g, "rating"): k_group_heads and the rest, at every cardinality
    docs    list_documents("uid < G", "rating") — a mask of as many members as g has values — its select / gather / sort beside top_groups' over G composites
Medians over the repetitions, the first left out.  The host times are taken under the trace, which slows the host: they are upper bounds.  COST_DOCS
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
ALL, TWO, ONE = "rating >= 1.0", "year >= 2000 AND rating > 7.0", "year = 1987 AND rating >= 1.0"
FILTERS = (("100 %", ALL), ("11 %", TWO), ("1.3 %", ONE))
GROUPS = (("g8", 8), ("g4000", 4000), ("g100k", 100000), ("uid", 0))
KERNELS = ("k_filter_mask_multi", "k_field_stats", "k_top_sizes", "k_top_keys", "k_top_hist", "k_top_pick", "k_top_gather", "k_top_page", "k_group_heads_mask", "k_group_heads",
           "k_group_page", "k_group_sizes", "k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort")
SELECT = ("k_top_hist", "k_top_pick")
LIST = ("k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort")


def kernel_of(name):
    for k in KERNELS:                                                  # (k_group_heads_mask before k_group_heads)
        if k in name:
            return k
    return None


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
    assert len(rows) >= need, "the trace holds fewer launches (%d) than the timed calls made (%d)" % (len(rows), need)
    rows = rows[len(rows) - need:]                                     # the timed calls are the last ones of the run
    by = {}
    at = 0
    for c in log["calls"]:
        seg = rows[at:at + c["launches"]]; at += c["launches"]
        if c["rep"] == 0:
            continue
        d = {}
        for _, k, us in seg:
            d[k] = d.get(k, 0.0) + us
        by.setdefault((c["case"], c["kind"]), []).append((d, c["ms"], c))
    med = lambda xs: float(np.median(xs)) if len(xs) else float("nan")
    print("| case | members | groups | table in | accumulate: k_field_stats of top_groups (us) | k_field_stats of field_stats (us) | k_top_sizes (us) | k_group_heads (us) | k_top_keys, sum (us) "
          "| 9 x k_top_hist + k_top_pick, sum (us) | k_top_keys, size (us) | 6 x hist + pick, size (us) | k_top_gather + k_top_page (us) | list_documents select + gather + sort over G members (us) "
          "| accumulate MB (flags + 2 x codes) | accumulate GB/s | composites MB per pass (sum) | top_groups call, sum / size (ms, under the trace) |")
    print("|" + "---|" * 18)
    for name in log["cases"]:
        get = lambda kind, ks: med([sum(d.get(k, 0.0) for k in ks) for d, _, _ in by.get((name, kind), [])])
        top = by[(name, "top")]
        c = top[0][2]
        acc = get("top", ("k_field_stats",))
        mb = (1 + 8 * c["share4"]) * DOCS / 1e6
        place = "LDS" if c["place"][0] else "LDS of a CU" if c["place"][1] else "global"
        print("| %s | %d | %d | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f | %.2f | %.3f / %.3f |" % (
            name, c["members"], c["groups"], place, acc, get("stats", ("k_field_stats",)), get("size", ("k_top_sizes",)), get("heads", ("k_group_heads",)),
            get("top", ("k_top_keys",)), get("top", SELECT), get("size", ("k_top_keys",)), get("size", SELECT), get("top", ("k_top_gather", "k_top_page")), get("docs", LIST),
            mb, mb * 1e6 / (acc * 1e-6) / 1e9, c["slots"] * 16 / 1e6, med([ms for _, ms, _ in top]), med([ms for _, ms, _ in by[(name, "size")]])))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine, TopGroupsRequest
    from tools.synth import Synth, config5_columns
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre = config5_columns(DOCS)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    rng = np.random.default_rng(7)
    cols = {}
    for g, card in GROUPS:
        cols[g] = rng.integers(0, card, DOCS).astype(np.int64) if card else rng.permutation(DOCS).astype(np.int64)
        e.set_column(g, cols[g], facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    share = {}
    for fname, x in FILTERS:                                           # warm: masks, sort rank, value table, group ranks; the share of 4-document groups with a member
        m = e.prefilter_mask(x)
        pad = np.ones((len(m) + 3) // 4 * 4, np.uint8); pad[:len(m)] = m
        share[x] = float((pad.reshape(-1, 4).min(axis=1) == 0).mean())
        for g, card in GROUPS:
            e.top_groups(x, g, "sum", "rating"); e.top_groups(x, g); e.list_groups(x, g, "rating", True, 0, 20)
            e.list_documents("uid < %d" % (card or DOCS), "rating", True, 0, 20)
            if card and card <= 4096:
                e.field_stats(x, "rating", g)
    # the answers, once, against the columns: the sums of g8 under the 1.3 % filter, largest first
    sel = (year == 1987) & (rating >= 1.0)
    got = e.top_groups(ONE, "g8", "sum", "rating", False, 0, 20)
    want = sorted(((math.fsum(rating[sel & (cols["g8"] == v)]), str(v)) for v in range(8)), key=lambda t: (-t[0], t[1]))
    assert [(r.sum, r.value) for r in got.groups] == want and got.total == int(sel.sum()), (got, want)
    st = e.field_stats(ALL, "rating", "g4000")
    tg = e.top_groups([TopGroupsRequest(ALL, "g4000", "size", "rating", False, off, 1024) for off in range(0, 4096, 1024)])
    assert [(r.value, r.count, r.sum, r.mean, r.min, r.max) for p in tg for r in p.groups] == [(s.value, s.count, s.sum, s.mean, s.min, s.max) for s in st.groups]
    print("the ranking equals the columns' sums; 4000 groups equal field_stats row for row", flush=True)
    log = {"cases": [], "calls": []}
    for g, card in GROUPS:
        for fname, x in FILTERS:
            name = "%s, %s" % (g, fname)
            log["cases"].append(name)
            G = card or DOCS
            for rep in range(REPS):
                def timed(kind, fn, launches):
                    t = time.perf_counter(); a = fn(); ms = (time.perf_counter() - t) * 1e3
                    rec = {"case": name, "kind": kind, "rep": rep, "ms": ms, "launches": launches()}
                    log["calls"].append(rec)
                    return a, rec
                a, rec = timed("top", lambda: e.top_groups(x, g, "sum", "rating", False, 0, 20), lambda: e.last_top_groups_stats()[4])
                assert e.last_top_groups_stats()[:3] == (0, 1, 1) and a.error is None
                rec.update({"members": a.total, "groups": a.total_groups, "place": list(e.last_top_groups_placement()), "share4": share[x], "slots": G})
                b, _ = timed("size", lambda: e.top_groups(x, g), lambda: e.last_top_groups_stats()[4])
                assert b.total_groups == a.total_groups
                if card and card <= 4096:
                    timed("stats", lambda: e.field_stats(x, "rating", g), lambda: e.last_field_stats_stats()[2])
                timed("heads", lambda: e.list_groups(x, g, "rating", True, 0, 20), lambda: e.last_group_list_stats()[4])
                timed("docs", lambda: e.list_documents("uid < %d" % G, "rating", True, 0, 20), lambda: e.last_list_stats()[3])
            print("PHASE %s: %d members, %d groups" % (name, a.total, a.total_groups), flush=True)
    if out_path:
        json.dump(log, open(out_path, "w"), indent=1)
