"""The launches behind the cost table of the browse scan in DESIGN 4 (run it under `rocprofv3 --kernel-trace`): 10 M documents, config-5 columns.

    python tools/bench_browse.py count           K = 1, 16, 256 uncounted expressions in text queries -> k_filter_count_multi
    python tools/bench_browse.py browse          the same expressions through browse queries -> k_browse_scan (uncounted, then with cached counts),
                                                 256 selective filters (no early stop possible), then facets_of_all_documents -> k_facets_all
    python tools/bench_browse.py count,browse    both in one process

Each case runs REPS times; restore_documents() voids the cached counts between repetitions.  INFX_BROWSE_EARLY_STOP=0 switches the rows-only early
stop off.  COST_DOCS overrides the corpus size.  Prints one marker line per repetition; the durations come from the kernel trace, in launch order."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infidex_amd import SearchEngine, Query  # noqa: E402
from tools.synth import Synth, config5_columns  # noqa: E402

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 4
modes = sys.argv[1].split(",")


def exprs(n, seed):
    rng = np.random.default_rng(seed)
    genres = ["Action", "Comedy", "Drama", "Horror", "Sci-Fi", "Romance", "Thriller", "Western"]
    out = []
    i = 0
    while len(out) < n:
        y = int(rng.integers(1950, 2024)); r = float(np.round(rng.uniform(1.0, 9.5), 1)); g = genres[int(rng.integers(len(genres)))]
        x = ["year >= %d AND rating > %.1f" % (y, r), "genre = '%s' OR year < %d" % (g, y), "rating BETWEEN %.1f AND %.1f" % (r, r + 1.0),
             "genre IN ('%s', 'Drama') AND year != %d" % (g, y)][i % 4]
        i += 1
        if x not in out:
            out.append(x)
    return out


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

for mode, K in [(m, k) for m in modes for k in (1, 16, 256)]:
    X = exprs(K, 100 + K)
    if mode == "count":
        qs = [Query(text, 10, filter=x) for x in X]
    else:
        qs = [Query("", 10, filter=x, enable_facets=True) for x in X]
    for rep in range(REPS):
        e.restore_documents()                                          # voids the count cache: every expression is counted again
        r = e.search_queries(qs)
        st = e.last_count_stats()
        print("PHASE %s uncounted K=%d rep=%d counted=%d fcm_launches=%d in_filter0=%d rows0=%d" % (mode, K, rep, st[0], st[1], r[0].total_in_filter, len(r[0].records)), flush=True)
    if mode == "browse":
        for rep in range(REPS):
            r = e.search_queries(qs)                                   # counts cached: rows only
            st = e.last_count_stats()
            print("PHASE browse cached K=%d rep=%d counted=%d rows0=%d" % (K, rep, st[0], len(r[0].records)), flush=True)
if "browse" in modes:
    # selective filters: rows deep in the corpus, where a rows-only scan cannot stop early
    sel = [Query("", 10, filter="year = %d AND rating = %.1f AND genre = 'Western'" % (1950 + i % 70, 1.0 + (i % 80) / 10.0), enable_facets=True) for i in range(256)]
    e.search_queries(sel)
    for rep in range(REPS):
        r = e.search_queries(sel)
        print("PHASE browse cached-selective K=256 rep=%d rows0=%d" % (rep, len(r[0].records)), flush=True)
    for rep in range(REPS):
        f = e.facets_of_all_documents()
        print("PHASE facets_all rep=%d fields=%s" % (rep, {k: len(v) for k, v in f.items()}), flush=True)
