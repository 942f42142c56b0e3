"""The calls and launches behind profiles/list_groups.md: list_groups at 10 M documents, config-5 columns (year 75 values, rating 91, genre 12) plus random
int group columns of 8, 100, 4000, 12 000 and 100 000 values (`g8` .. `g100k`) and a unique one (`uid`).  Two runs, because a kernel trace slows the host:

    python tools/bench_list_groups.py --out calls.json                                      # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_list_groups.py
    python tools/bench_list_groups.py --summarize trace/<host>/<pid>_kernel_trace.csv calls.json > profiles/list_groups.md

Cases: one page (offset 0, limit 20, order by `rating`, ascending) grouped by each of the six columns under `rating >= 1.0` (every document),
`year >= 2000 AND rating > 7.0` (11 %) and `year = 1987 AND rating >= 1.0` (1.3 %); and sixteen consecutive pages of 20 of the 11 % listing by g4000 in one call.
The head table of g8, g100 and g4000 lies in a workgroup's LDS, g12k's in the whole LDS of a CU, g100k's and uid's in global memory.

Every repetition starts a new mask epoch (restore_documents) and asks the same request twice: the first call builds its mask in front ("cold": the
k_filter_mask_multi launch of that call is the case's yardstick, in the same trace), the second finds it ("cached").  With --out the same pair is timed for
list_documents with the same filter, order and limit.  The first repetition of a case is left out; medians.  COST_DOCS overrides the corpus size."""
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
GROUPS = (("g8", 8, "LDS"), ("g100", 100, "LDS"), ("g4000", 4000, "LDS"), ("g12k", 12000, "LDS of a CU"), ("g100k", 100000, "global"), ("uid", 0, "global"))
ORDER = "rating"
LIST_KERNELS = ("k_list_hist", "k_list_pick", "k_list_count", "k_list_prefix", "k_list_gather", "k_list_sort")
KERNELS = ("k_filter_mask_multi", "k_group_heads_mask", "k_group_heads", "k_group_page", "k_group_sizes") + LIST_KERNELS


def cases():
    """name -> (filter name, filter, group column, pages)"""
    out = {}
    for g, _, _ in GROUPS:
        for fname, x in FILTERS:
            out["%s, %s" % (g, fname)] = (fname, x, g, 1)
    out["g4000, 11 %, sixteen pages"] = ("11 %", TWO, "g4000", 16)
    return out


def requests(x, g, pages):
    from infidex_amd import GroupListRequest
    return [GroupListRequest(x, g, ORDER, True, 20 * p, 20) for p in range(pages)]


def kernel_of(name):
    for k in KERNELS:                                                  # (k_group_heads_mask before k_group_heads)
        if k in name:
            return k
    return None


def summarize(path, calls_path=None):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            k = kernel_of(r["Kernel_Name"])
            if k:
                rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    # one list_groups call of this tool: [k_filter_mask_multi] k_group_heads ... (a single spec per call)
    calls, prev = [], None
    for _, k, d in rows:
        if k == "k_filter_mask_multi" or (k == "k_group_heads" and prev != "k_filter_mask_multi"):
            calls.append({})
        if calls:
            calls[-1].setdefault(k, []).append(d)
        prev = k
    warm = 1                                                           # the call that builds the order column's sort rank
    want = warm + 2 * REPS * len(cases())
    assert len(calls) == want, "the trace does not hold the launches of one run of this tool (%d calls, %d expected)" % (len(calls), want)
    host = json.load(open(calls_path)) if calls_path else {}
    print("| case | table in | members | groups | k_filter_mask_multi (us) | k_group_heads (us) | heads / mask build | k_group_heads_mask (us) | select + gather + sort (us) | k_group_page (us) "
          "| k_group_sizes (us) | all kernels, cached (us) | MB of the head pass (flags + group codes + order codes) | + rank gather MB | head pass GB/s | members / us "
          "| list_groups call, cached / cold (ms) | list_documents call, cached / cold (ms) |")
    print("|" + "---|" * 18)
    at = warm
    for name, (fname, x, g, pages) in cases().items():
        seg = calls[at:at + 2 * REPS]; at += 2 * REPS
        cold, cached = seg[2::2], seg[3::2]                            # (the first repetition left out)
        assert all("k_filter_mask_multi" in c for c in cold) and not any("k_filter_mask_multi" in c for c in cached), name
        med = lambda cs, k: float(np.median([sum(c.get(k, [0.0])) for c in cs]))
        mask = med(cold, "k_filter_mask_multi"); heads = med(cold + cached, "k_group_heads"); hm = med(cold + cached, "k_group_heads_mask")
        lst = float(np.median([sum(sum(c.get(k, [])) for k in LIST_KERNELS) for c in cold + cached]))
        page, sizes = med(cold + cached, "k_group_page"), med(cold + cached, "k_group_sizes")
        total = float(np.median([sum(sum(v) for v in c.values()) for c in cached]))
        h = host.get(name, {})
        place = [p for gg, _, p in GROUPS if gg == g][0]
        if h:
            mb = (1 + 8 * h["share4"]) * DOCS / 1e6; gather = 4 * h["members"] / 1e6
            extra = "| %.1f | %.1f | %.0f | %.0f | %.3f / %.3f | %.3f / %.3f |" % (mb, gather, (mb + gather) * 1e6 / (heads * 1e-6) / 1e9, h["members"] / heads,
                                                                                  h["cached"], h["cold"], h["doc_cached"], h["doc_cold"])
            head = "| %s | %s | %d | %d " % (name, place, h["members"], h["groups"])
        else:
            extra, head = "| - | - | - | - | - | - |", "| %s | %s | - | - " % (name, place)
        print(head + "| %.1f | %.1f | %.2f | %.1f | %.1f | %.1f | %.1f | %.1f " % (mask, heads, heads / mask, hm, lst, page, sizes, total) + extra)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine, ListRequest
    from tools.synth import Synth, config5_columns
    t0 = time.time()
    syn = Synth(5, docs=DOCS)
    arena, offs = syn.docs()
    e = SearchEngine.create_default(device=0)
    e.index_flat(None, arena, offs, syn.field_weights)
    year, rating, genre = config5_columns(DOCS)
    e.set_column("year", year, facetable=True); e.set_column("rating", rating, facetable=False); e.set_column("genre", genre, facetable=True)
    rng = np.random.default_rng(7)
    for g, card, _ in GROUPS:
        e.set_column(g, rng.integers(0, card, DOCS).astype(np.int64) if card else rng.permutation(DOCS).astype(np.int64), facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    t = time.perf_counter()
    first = e.list_groups(None, "g8", ORDER, True, 0, 20)             # the sort rank is built on first use: outside the timed calls
    print("first use of %s: %.1f ms; %d groups of %d documents" % (ORDER, (time.perf_counter() - t) * 1e3, first.total_groups, first.total), flush=True)
    calls = {}
    for name, (fname, x, g, pages) in cases().items():
        reqs = requests(x, g, pages)
        cold, cached = [], []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch
            t = time.perf_counter(); a = e.list_groups(reqs); cold.append(time.perf_counter() - t)
            assert e.last_group_list_stats()[:3] == (1, 0, 1)
            t = time.perf_counter(); b = e.list_groups(reqs); cached.append(time.perf_counter() - t)
            assert e.last_group_list_stats()[:3] == (0, 1, 1) and repr(a) == repr(b) and all(p.error is None for p in a)
        calls[name] = {"cold": float(np.median(cold[1:])) * 1e3, "cached": float(np.median(cached[1:])) * 1e3, "members": a[0].total, "groups": a[0].total_groups}
        print("PHASE %s: %d members, %d groups, cached %.3f ms, cold %.3f ms" % (name, a[0].total, a[0].total_groups, calls[name]["cached"], calls[name]["cold"]), flush=True)
    if out_path:                                                       # profiler-off run only: list_documents beside it, and the share of the 4-document groups with a member
        share = {}
        for fname, x in FILTERS:
            m = e.prefilter_mask(x)
            pad = np.ones((len(m) + 3) // 4 * 4, np.uint8); pad[:len(m)] = m
            share[x] = float((pad.reshape(-1, 4).min(axis=1) == 0).mean())
        for name, (fname, x, g, pages) in cases().items():
            reqs = [ListRequest(x, ORDER, True, 20 * p, 20) for p in range(pages)]
            cold, cached = [], []
            for rep in range(REPS):
                e.restore_documents()
                t = time.perf_counter(); e.list_documents(reqs); cold.append(time.perf_counter() - t)
                t = time.perf_counter(); e.list_documents(reqs); cached.append(time.perf_counter() - t)
            calls[name].update({"doc_cold": float(np.median(cold[1:])) * 1e3, "doc_cached": float(np.median(cached[1:])) * 1e3, "share4": share[x]})
            print("PHASE %s: list_documents cached %.3f ms, cold %.3f ms" % (name, calls[name]["doc_cached"], calls[name]["doc_cold"]), flush=True)
        # the answer, once, against the columns: the heads of g100 under the 1.3 % filter
        sel = np.nonzero((year == 1987) & (rating >= 1.0))[0]
        got = e.list_groups(ONE, "g8", None, True, 0, 20)
        assert got.total == len(sel) and got.total_groups == 8 and sum(got.group_sizes) == len(sel), (got.total, len(sel))
        print("totals and sizes equal the columns' counts", flush=True)
        json.dump(calls, open(out_path, "w"), indent=1)
