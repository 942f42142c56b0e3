"""The launches behind profiles/list_columns.md: k_list_leaf beside k_filter_mask_multi, k_list_facets beside k_facets_filtered, 10 M documents.
Run it under `rocprofv3 --kernel-trace --output-format csv`, then hand the trace to --summarize:

    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_list_columns.py
    python tools/bench_list_columns.py --summarize trace/<host>/<pid>_kernel_trace.csv

The corpus: a scalar column `year` (75 values), a facetable scalar column `genre` (12 values) and a facetable list column `tags` of ints 0 .. 999 with
0 .. 6 elements per document (mean 3: E = 30 M elements).  Every repetition starts a new mask epoch, empties the filter cache of what holds a derived
column and uses leaves the engine has not seen, so nothing is answered from a cache; per repetition, in this order:
    prefilter_mask("year = Y")                      k_filter_mask_multi over one scalar column (the yardstick of k_list_leaf)
    prefilter_mask("tags = a")                      k_list_leaf K = 1, then k_filter_mask_multi over the derived column
    prefilter_mask("tags = a1 OR .. OR tags = a16") k_list_leaf K = 16, then k_filter_mask_multi over sixteen derived columns
    facets_of_documents(["year = Y"])               k_facets_filtered K = 1 with one facet column, then the mask and k_list_facets K = 1
    facets_of_documents([16 x "year = Yi"])         k_facets_filtered K = 16, the masks, k_list_facets K = 16
The first repetition is left out of the summary; the median of the others is reported with the bytes each kernel has to move — k_list_leaf reads
4 (n + 1) + 4 E and writes 4 K n; k_list_facets reads 4 (n + 1) + 4 E + K n; k_filter_mask_multi over one column reads 5 n and writes n; k_facets_filtered
reads two columns and the Deleted flags, 9 n — and that bound's share of the time at the HBM peak.  COST_DOCS overrides the corpus size."""
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 5
HBM_PEAK = 8.0e12                      # bytes per second (MI355X)
KERNELS = ("k_list_leaf", "k_list_facets", "k_filter_mask_multi", "k_facets_filtered")
# the kernels of interest of one repetition, in launch order, with what they are in the table
REP = [("k_filter_mask_multi", "flush"), ("k_filter_mask_multi", "scalar K=1"), ("k_list_leaf", "K=1"), ("k_filter_mask_multi", "derived K=1"),
       ("k_filter_mask_multi", "flush"), ("k_list_leaf", "K=16"), ("k_filter_mask_multi", "derived K=16"), ("k_facets_filtered", "K=1"), ("k_filter_mask_multi", "facet masks K=1"),
       ("k_list_facets", "K=1"), ("k_facets_filtered", "K=16"), ("k_filter_mask_multi", "facet masks K=16"), ("k_list_facets", "K=16")]


def lengths(n):
    return np.random.default_rng(7).integers(0, 7, n).astype(np.uint64)


def summarize(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    us = {}
    for k in KERNELS:                                                  # each kernel's launches in order: the cases of a repetition follow one another
        mine = [d for _, kk, d in rows if kk == k]; cases = [c for kk, c in REP if kk == k]
        assert len(mine) == len(cases) * REPS, "the trace does not hold the launches of one run of this tool (%s: %d launches, %d expected)" % (k, len(mine), len(cases) * REPS)
        for i, d in enumerate(mine):
            if i >= len(cases):                                        # the first repetition is left out
                us.setdefault((k, cases[i % len(cases)]), []).append(d)
    n, E = DOCS, int(lengths(DOCS).sum())
    csr = 4 * (n + 1) + 4 * E
    table = [("k_filter_mask_multi", "scalar K=1", 6 * n), ("k_list_leaf", "K=1", csr + 4 * n), ("k_list_leaf", "K=16", csr + 64 * n),
             ("k_filter_mask_multi", "derived K=1", 6 * n), ("k_filter_mask_multi", "derived K=16", 65 * n + 16 * n),
             ("k_facets_filtered", "K=1", 9 * n), ("k_list_facets", "K=1", csr + n), ("k_facets_filtered", "K=16", 9 * n), ("k_list_facets", "K=16", csr + 16 * n)]
    print("%d documents, %d elements" % (n, E))
    print("| kernel | case | us (median of %d) | min - max (us) | bytes (MB) | byte bound (us) | bound / time |" % (REPS - 1))
    print("|---|---|---|---|---|---|---|")
    for k, case, b in table:
        t = float(np.median(us[(k, case)])); bound = b / HBM_PEAK * 1e6
        print("| %s | %s | %.1f | %.1f - %.1f | %.1f | %.1f | %.2f |" % (k, case, t, min(us[(k, case)]), max(us[(k, case)]), b / 1e6, bound, bound / t))


def add_int_list_column(e, name, lens, values, facetable):
    """set_list_column from arrays: ten million Python lists are not what is measured here."""
    offs = np.zeros(len(lens) + 1, np.uint64); offs[1:] = np.cumsum(lens, dtype=np.uint64)
    v = np.ascontiguousarray(values, np.int64)
    e._check(e.L.infx_engine_add_list_column(e.h, name.encode(), 1, int(facetable), C.c_int64(len(lens)), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             v.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None))


def flush(e, expr):
    """No cached filter holds a derived column afterwards: the cache shrinks to one entry, which a scalar expression then takes (one k_filter_mask_multi launch)."""
    e.set_filter_cache_limit(1); e.prefilter_mask(expr); e.set_filter_cache_limit(4096)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
        sys.exit(0)
    from infidex_amd import SearchEngine
    from tools.synth import Synth, config5_columns
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, _, genre = config5_columns(DOCS)
    e.set_column("year", year, facetable=False); e.set_column("genre", genre, facetable=True)
    lens = lengths(DOCS)
    add_int_list_column(e, "tags", lens, np.random.default_rng(8).integers(0, 1000, int(lens.sum())), True)
    years = sorted(set(int(y) for y in year[:100000]))
    print("built in %.1f s: %d elements" % (time.time() - t0, int(lens.sum())), flush=True)
    for rep in range(REPS):
        e.restore_documents()                                          # a new mask epoch: masks and filtered facets are computed again
        flush(e, "year >= %d" % rep)
        m0 = e.prefilter_mask("year = %d" % years[rep])
        m1 = e.prefilter_mask("tags = %d" % rep)
        s1 = e.last_list_leaf_stats()
        flush(e, "year > %d" % rep)                                    # (sixteen derived columns are all the engine keeps)
        m16 = e.prefilter_mask(" OR ".join("tags = %d" % (100 + 16 * rep + i) for i in range(16)))
        s16 = e.last_list_leaf_stats()
        assert s1 == (1, 1) and s16 == (16, 1), (s1, s16)
        f1 = e.facets_of_documents(["year = %d" % years[20 + rep]])      # (expressions whose masks the session does not hold yet)
        f16 = e.facets_of_documents(["year = %d" % years[30 + rep + i] for i in range(16)])
        assert f1[0].error is None and all(f.error is None and f.total > 0 for f in f16) and e.last_filtered_facet_stats() == (16, 0, 1)
        print("PHASE rep=%d accepted: year %d, one tag %d, sixteen tags %d; tags facet %s" % (rep, int((m0 == 0).sum()), int((m1 == 0).sum()), int((m16 == 0).sum()),
                                                                                             f1[0].facets["tags"][:2]), flush=True)
