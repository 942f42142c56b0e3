"""The calls and launches behind profiles/list_documents.md: list_documents at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus a
unique int column (`uid`).  Two runs, because a kernel trace slows the host:

    python tools/bench_list_documents.py --out calls.json                                     # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_list_documents.py
    python tools/bench_list_documents.py --summarize trace/<host>/<pid>_kernel_trace.csv [calls.json]

Cases: filters `rating >= 1.0` (every document; also the one-column program whose k_filter_mask_multi launch is the yardstick of a histogram pass),
`year >= 2000 AND rating > 7.0` and `year = 1987 AND rating >= 1.0` (about 1.3 %); order by year (one 11-bit pass), rating (one) and uid (24 bits: three);
offsets 0 and deep — 1 000 000, or half the set where the set is smaller than 2 000 000 (the claim: the offset does not change the time); limits 20 and 1024.  Every repetition starts a new mask epoch
(restore_documents) and lists the same page twice: the first call builds the mask (cold), the second finds it (cached).  The first repetition of a case is
left out, the median of the others is reported, cold and cached calls apart.  Algorithmic bytes of a histogram or count pass: (1 + 4 x share of the 4-document groups that hold an
accepted document) x documents, plus the rank gather (4 bytes per accepted document, from a table of 4 x distinct values bytes).  COST_DOCS overrides the
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
FILTERS = [("all", "rating >= 1.0"), ("two-column", "year >= 2000 AND rating > 7.0"), ("1 %", "year = 1987 AND rating >= 1.0")]
ORDERS = ["year", "rating", "uid"]
OFFSETS = ["0", "deep"]
LIMITS = [20, 1024]
KERNELS = ("k_filter_mask_multi", "k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort")


def passes(nvals, bits=11):
    return ((nvals + 1).bit_length() + bits - 1) // bits


def offset_of(label, total):
    """the offset of a case: 0, or a deep one that lies inside the set"""
    return 0 if label == "0" else (1000000 if total >= 2000000 else total // 2)


def cases():
    return [(f, o, off, lim) for f in FILTERS for o in ORDERS for off in OFFSETS for lim in LIMITS]


def sequence(nvals):
    """The kernels in launch order: (case, rep, cold, kernel)."""
    out = []
    for o in ORDERS:                                                   # the calls that build the sort ranks
        out += [(None, 0, False, k) for k in ["k_list_hist", "k_list_pick"] * passes(nvals[o]) + ["k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort"]]
    for _ in FILTERS:                                                  # the calls that ask for the sets' sizes (index order: one pass), each building its mask
        out += [(None, 0, True, k) for k in ["k_filter_mask_multi", "k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort"]]
    for c in cases():
        p = passes(nvals[c[1]])
        for rep in range(REPS):
            for cold in (True, False):
                ks = (["k_filter_mask_multi"] if cold else []) + ["k_list_hist", "k_list_pick"] * p + ["k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort"]
                out += [(c, rep, cold, k) for k in ks]
    return out


def columns():
    from tools.synth import config5_columns
    year, rating, genre = config5_columns(DOCS)
    uid = np.random.default_rng(7).permutation(np.arange(DOCS, dtype=np.int64))
    return year, rating, genre, uid


def shares(year, rating):
    """per filter: (share of documents accepted, share of 4-document groups with an accepted document)"""
    acc = {"all": rating >= 1.0, "two-column": (year >= 2000) & (rating > 7.0), "1 %": (year == 1987) & (rating >= 1.0)}
    out = {}
    for k, a in acc.items():
        pad = np.concatenate([a, np.zeros((-len(a)) % 4, bool)]).reshape(-1, 4)
        out[k] = (float(a.mean()), float(pad.any(axis=1).mean()))
    return out


def summarize(path, calls_path=None):
    year, rating, genre, uid = columns()
    nvals = {"year": len(np.unique(year)), "rating": len(np.unique(rating)), "uid": DOCS}
    sh = shares(year, rating)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    seq = sequence(nvals)
    assert [k for _, k, _ in rows] == [s[3] for s in seq], "the trace does not hold the launches of one run of this tool (%d launches, %d expected)" % (len(rows), len(seq))
    us = {}
    for (c, rep, cold, kern), (_, _, d) in zip(seq, rows):
        if rep:
            us.setdefault((c, kern), {}).setdefault((rep, cold), []).append(d)
    calls = json.load(open(calls_path)) if calls_path else {}

    def med(c, kern, cold, each=False):
        per = [v for (rep, cd), v in us.get((c, kern), {}).items() if cd == cold]
        return float(np.median([x[0] if each else sum(x) for x in per])) if per else 0.0
    print("| filter | accepted | order by | passes | offset | limit | masks | call (ms) | k_filter_mask_multi (us) | k_list_hist per pass (us) | k_list_pick (us) | "
          "k_list_count (us) | k_list_prefix (us) | k_list_gather (us) | k_list_sort (us) | MB per hist / count pass (flags + codes) | + rank gather MB | hist GB/s |")
    print("|" + "---|" * 18)
    for c in cases():
        (fname, _), o, off, lim = c
        p = passes(nvals[o])
        mb = DOCS * (1 + 4 * sh[fname][1]) / 1e6
        gather = DOCS * sh[fname][0] * 4 / 1e6
        cc = calls.get("%s|%s|%s|%d" % (fname, o, off, lim), {})
        for cold in (True, False):
            hist = [float(np.median([x[i] for (rep, cd), x in us[(c, "k_list_hist")].items() if cd == cold])) for i in range(p)]
            print("| %s | %.3f | %s | %d | %d | %d | %s | %s | %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f |" % (
                fname, sh[fname][0], o, p, offset_of(off, int(round(sh[fname][0] * DOCS))), lim, "cold" if cold else "cached",
                "%.3f" % cc["cold" if cold else "cached"] if cc else "-", "%.1f" % med(c, "k_filter_mask_multi", True) if cold else "-",
                " / ".join("%.1f" % h for h in hist), med(c, "k_list_pick", cold, True), med(c, "k_list_count", cold), med(c, "k_list_prefix", cold), med(c, "k_list_gather", cold),
                med(c, "k_list_sort", cold), mb, gather, (mb + gather) / 1e3 / (float(np.mean(hist)) * 1e-6)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine
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
    for o in ORDERS:                                                   # the sort ranks are built on first use: outside the timed calls
        e.list_documents(None, o, True, 0, 1)
    calls = {}
    totals = {fname: e.list_documents(x, None, True, 0, 1).total for fname, x in FILTERS}
    for (fname, x), o, label, lim in cases():
        off = offset_of(label, totals[fname])
        cold, cached = [], []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch: the next call builds its mask
            t = time.perf_counter(); a = e.list_documents(x, o, True, off, lim); cold.append(time.perf_counter() - t)
            assert e.last_list_stats()[:2] == (1, 0)
            t = time.perf_counter(); b = e.list_documents(x, o, True, off, lim); cached.append(time.perf_counter() - t)
            assert e.last_list_stats()[:2] == (0, 1) and a == b and a.error is None
        key = "%s|%s|%s|%d" % (fname, o, label, lim)
        calls[key] = {"offset": off, "cold": float(np.median(cold[1:])) * 1e3, "cached": float(np.median(cached[1:])) * 1e3, "total": a.total, "rows": len(a.document_ids)}
        print("PHASE %s by %s offset %d limit %d: total %d rows %d passes %d cold %.3f ms cached %.3f ms" % (
            fname, o, off, lim, a.total, len(a.document_ids), e.last_list_stats()[2], calls[key]["cold"], calls[key]["cached"]), flush=True)
    if out_path:
        json.dump(calls, open(out_path, "w"), indent=1)
