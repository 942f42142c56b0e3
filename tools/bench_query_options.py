"""Throughput of per-query options (infx_engine_set_query_options) against the session-wide filter, config 5.

Three cases over the same 1000-query batches, `--sessions` host threads with one engine session each:
  (i)   the config-5 filter + facets installed once per session (Session.set_filter), plain batches;
  (ii)  the same filter + facets given per query;
  (iii) per query, a filter drawn from a pool of `--pool` expressions (or none), facets on half, boosts or a sort on a third.
The batches of (iii) that count the pool's expressions for the first time (NumberOfDocumentsInFilter, k_filter_count_multi) are timed on their own
before the steady state.  Prints one JSON line.
  (iv)  with --wide-leg: the engine is created with max_post_rows=1024 and every query of the same batches asks WIDE_K = 500 rows (coverage off) with
        the config-5 filter, facets and a sort-by — the workgroup-per-query kernels (k_postfilter_wide, k_postproc_wide), whose serial sort of up to
        500 rows is paid per query.  Cases (i)-(iii) run first, on the same engine: their queries stay on the one-wave kernels.

    python tools/bench_query_options.py [--docs N] [--steps 20] [--warmup 4] [--sessions 4] [--pool 200] [--wide-leg]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infidex_amd import SearchEngine, Query, Boost, BoostStrength  # noqa: E402
from infidex_amd.engine import Session, pack_texts, _install_query_options  # noqa: E402
from tools.synth import Synth, config5_columns  # noqa: E402

K = 20
WIDE_K = 500


def pool_exprs(n, seed=3):
    rng = np.random.default_rng(seed)
    genres = ["Action", "Comedy", "Drama", "Horror", "Sci-Fi", "Romance", "Thriller", "Western"]
    out = []
    for i in range(n):
        y = int(rng.integers(1950, 2024)); r = float(np.round(rng.uniform(1.0, 9.5), 1)); g = genres[int(rng.integers(len(genres)))]
        out.append(["year >= %d AND rating > %.1f" % (y, r), "genre = '%s' OR year < %d" % (g, y), "rating BETWEEN %.1f AND %.1f" % (r, r + 1.0),
                    "genre IN ('%s', 'Drama') AND year != %d" % (g, y)][i % 4])
    return list(dict.fromkeys(out))[:n]


def run(sessions, batches, prep, k=K, coverage=True):
    """Every batch through `prep(session, i)` (installs its options; returns the packed texts) and search_packed; returns seconds."""
    cur = {"i": 0}; lock = threading.Lock(); err = []

    def worker(se):
        try:
            while True:
                with lock:
                    i = cur["i"]; cur["i"] += 1
                if i >= len(batches):
                    return
                arena, offs = prep(se, i)
                se.search_packed(arena, offs, k, 500, coverage)
        except Exception as ex:
            err.append(ex)

    t0 = time.time()
    ths = [threading.Thread(target=worker, args=(se,)) for se in sessions]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if err:
        raise err[0]
    return time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--sessions", type=int, default=4)
    ap.add_argument("--pool", type=int, default=200)
    ap.add_argument("--wide-leg", action="store_true", help="add case (iv): 500 rows per query with filter, facets and sort-by (max_post_rows=1024)")
    args = ap.parse_args()
    syn = Synth(5, docs=args.docs)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0, **({"max_post_rows": 1024} if args.wide_leg else {})); e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre = config5_columns(args.docs)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    flt = syn.cfg["filter"]
    n = args.warmup + args.steps
    qa, qo = syn.queries(n * args.batch, qseed=1000)
    texts = Synth.texts(qa, qo)
    tb = [texts[i * args.batch:(i + 1) * args.batch] for i in range(n)]
    packed = [pack_texts(t) for t in tb]
    sessions = [Session(e) for _ in range(args.sessions)]
    out = {"docs": args.docs, "batch": args.batch, "steps": args.steps, "sessions": args.sessions, "filter": flt}

    # (i) session-wide filter + facets
    for se in sessions:
        se.set_filter(flt, True)
    run(sessions, packed[:args.warmup], lambda se, i: packed[i])
    dt = run(sessions, packed[args.warmup:], lambda se, i: packed[args.warmup + i])
    out["i_session_filter_qps"] = args.steps * args.batch / dt
    for se in sessions:
        se.set_filter(None)

    # (ii) the same filter + facets per query
    same = [[Query(t, K, filter=flt, enable_facets=True) for t in b] for b in tb]

    def prep2(se, i, off=0):
        _install_query_options(e, se.h, same[off + i]); return packed[off + i]
    run(sessions, packed[:args.warmup], prep2)
    dt = run(sessions, packed[args.warmup:], lambda se, i: prep2(se, i, args.warmup))
    out["ii_per_query_same_filter_qps"] = dt and args.steps * args.batch / dt

    # (iii) a per-query mix from a pool of expressions; boosts or a sort on a third of the queries
    pool = pool_exprs(args.pool)
    rng = np.random.default_rng(9)
    boosts = [Boost("year >= 2010", BoostStrength.High), Boost("genre = 'Drama'", BoostStrength.Low)]

    def mixq(t, j):
        x = int(rng.integers(0, 3))
        return Query(t, K, filter=None if rng.random() < 0.1 else pool[int(rng.integers(len(pool)))], enable_facets=bool(rng.random() < 0.5),
                     enable_boost=x == 1, boosts=boosts if x == 1 else None, sort_by="year" if x == 2 else None, sort_ascending=bool(j & 1))
    mix = [[mixq(t, j) for j, t in enumerate(b)] for b in tb]
    first = [[Query(t, K, filter=pool[(j * 7 + i) % len(pool)]) for j, t in enumerate(b)] for i, b in enumerate(tb[:args.sessions])]
    t0 = time.time()
    counted = []

    def prep_first(se, i):
        _install_query_options(e, se.h, first[i]); return packed[i]
    run(sessions, packed[:len(first)], prep_first)
    out["iii_first_use_batches"] = len(first)
    out["iii_first_use_s"] = time.time() - t0
    for se in sessions:
        counted.append(se.last_count_stats())
    out["iii_first_use_counted_launches_per_session"] = counted

    def prep3(se, i, off=0):
        _install_query_options(e, se.h, mix[off + i]); return packed[off + i]
    run(sessions, packed[:args.warmup], prep3)
    dt = run(sessions, packed[args.warmup:], lambda se, i: prep3(se, i, args.warmup))
    out["iii_per_query_mix_qps"] = args.steps * args.batch / dt
    out["ii_over_i"] = out["ii_per_query_same_filter_qps"] / out["i_session_filter_qps"]
    out["iii_over_i"] = out["iii_per_query_mix_qps"] / out["i_session_filter_qps"]

    if args.wide_leg:       # (iv) 500 rows per query, coverage off, filter + facets + sort-by on every query
        widq = [[Query(t, WIDE_K, enable_coverage=False, filter=flt, enable_facets=True, sort_by="year", sort_ascending=bool(j & 1)) for j, t in enumerate(b)] for b in tb]

        def prep4(se, i, off=0):
            _install_query_options(e, se.h, widq[off + i]); return packed[off + i]
        run(sessions, packed[:args.warmup], prep4, WIDE_K, False)
        dt = run(sessions, packed[args.warmup:], lambda se, i: prep4(se, i, args.warmup), WIDE_K, False)
        out["iv_wide_rows"] = WIDE_K
        # how many rows the wide kernels actually worked on: one batch plain (the rows before the filter) and with the options
        se = sessions[0]
        before = se.search_packed(*packed[0], WIDE_K, 500, False)[3]
        after = se.search_packed(*prep4(se, 0), WIDE_K, 500, False)[3]
        out["iv_mean_rows_before_filter"] = float(before.mean()); out["iv_max_rows_before_filter"] = int(before.max())
        out["iv_mean_rows_returned"] = float(after.mean())
        out["iv_wide_500_rows_filter_facets_sort_qps"] = args.steps * args.batch / dt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
