"""The launches behind the cost table of the filtered facets in DESIGN 4 and profiles/filtered_facets.md: 10 M documents, config-5 columns (year and
genre facetable, rating not).  Run it under `rocprofv3 --kernel-trace --output-format csv`, then hand the trace to --summarize:

    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_filtered_facets.py
    python tools/bench_filtered_facets.py --summarize trace/<host>/<pid>_kernel_trace.csv

For K = 1, 4, 16 and two kinds of filter — selective (about 1.3 % of the documents each) and one every document passes — each repetition asks, for the
same K expressions, the three kernels whose times the table compares:
    k_filter_count_multi   the K expressions as Query.filter of K text queries (NumberOfDocumentsInFilter, one launch)
    k_facets_all           K times facets_of_all_documents (what K separate facet passes cost)
    k_facets_filtered      facets_of_documents of the K expressions (one launch)
restore_documents() starts a new mask epoch between repetitions, so nothing is answered from a cache.  The first repetition of a case is left out of
the summary.  All expressions read year and rating and the facets count year and genre: the fused kernel reads 3 columns + the Deleted flag = 13 bytes
per document, the count pass 2 columns + 1, a facet pass 2 columns + 1.  A second part adds a facetable column of 4000 values (`bucket`) and repeats K = 1
and 4: its K x 4000 counter words take the LDS budget (80 KiB per workgroup with the codes at K = 4, two workgroups per CU), the regime the small config-5
dictionaries never reach; there the fused kernel reads 4 columns = 17 bytes per document and a facet pass 3 columns.  COST_DOCS overrides the corpus size."""
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 5
KS = (1, 4, 16)
CASES = [("selective", KS, 3), ("everything", KS, 3), ("selective+4000", (1, 4), 4), ("everything+4000", (1, 4), 4)]      # (kind, Ks, columns the fused kernel reads)
KERNELS = ("k_filter_count_multi", "k_facets_all", "k_facets_filtered")


def exprs(kind, K):
    if kind.startswith("selective"):
        return ["year = %d AND rating >= 1.0" % (1960 + 3 * i) for i in range(K)]          # one year of 75: 1.3 % of the documents
    return ["rating >= 1.0 OR year = %d" % (1960 + 3 * i) for i in range(K)]               # every document


def sequence():
    """The kernels of interest in launch order: (kind, K, rep, kernel)."""
    out = []
    for kind, ks, _ in CASES:
        for K in ks:
            for rep in range(REPS):
                out.append((kind, K, rep, "k_filter_count_multi"))
                out += [(kind, K, rep, "k_facets_all")] * K
                out.append((kind, K, rep, "k_facets_filtered"))
    return out


def summarize(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for k in KERNELS:
                if k in name:
                    rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    seq = sequence()
    assert [k for _, k, _ in rows] == [s[3] for s in seq], "the trace does not hold the launches of one run of this tool (%d launches, %d expected)" % (len(rows), len(seq))
    us = {}
    for (kind, K, rep, kern), (_, _, d) in zip(seq, rows):
        if rep:                                                        # the first launch of a case is left out
            us.setdefault((kind, K, kern), {}).setdefault(rep, 0.0)
            us[(kind, K, kern)][rep] += d                              # (the K k_facets_all launches of a repetition add up)
    med = lambda kind, K, kern: float(np.median(list(us[(kind, K, kern)].values())))
    gb = lambda cols: DOCS * (cols * 4 + 1) / 1e9
    yard = lambda kind, K: (DOCS * 9 + K * DOCS * (13 if "+" in kind else 9)) / 1e9      # the two existing passes: count (2 columns) + K facet passes
    print("| filter | K | k_filter_count_multi (us) | K x k_facets_all (us) | sum (us) | sum GB | k_facets_filtered (us) | fused / sum | fused GB | fused TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for kind, ks, cols in CASES:
        for K in ks:
            c, a, f = med(kind, K, "k_filter_count_multi"), med(kind, K, "k_facets_all"), med(kind, K, "k_facets_filtered")
            print("| %s | %d | %.1f | %.1f | %.1f | %.3f | %.1f | %.2f | %.3f | %.2f |" % (kind, K, c, a, c + a, yard(kind, K), f, f / (c + a), gb(cols), gb(cols) / 1e3 / (f * 1e-6)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
        sys.exit(0)
    from infidex_amd import SearchEngine, Query
    from tools.synth import Synth, config5_columns
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre = config5_columns(DOCS)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    qa, qo = syn.queries(4, qseed=43, fuzz=0.0)
    text = Synth.texts(qa, qo)[0]
    print("built in %.1f s" % (time.time() - t0), flush=True)
    for kind, ks, _ in CASES:
        if kind == "selective+4000":
            e.set_column("bucket", np.random.default_rng(3).integers(0, 4000, DOCS).astype(np.int64), facetable=True)
        for K in ks:
            X = exprs(kind, K)
            for rep in range(REPS):
                e.restore_documents()                                  # a new mask epoch: counts and filtered facets are computed again
                r = e.search_queries([Query(text, 10, filter=x) for x in X])
                cs = e.last_count_stats()
                for _ in range(K):
                    allf = e.facets_of_all_documents()
                ff = e.facets_of_documents(X)
                st = e.last_filtered_facet_stats()
                assert cs == (K, 1) and st == (K, 0, 1), (cs, st)
                assert [f.total for f in ff] == [x.total_in_filter for x in r]
                if kind.startswith("everything"):
                    assert all(f.facets == allf and f.total == DOCS for f in ff)
                print("PHASE %s K=%d rep=%d total0=%d year0=%s" % (kind, K, rep, ff[0].total, ff[0].facets["year"][:1]), flush=True)
