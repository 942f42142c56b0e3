"""The calls and launches behind profiles/group_members.md: list_group_members at 10 M documents, on tools/bench_list_groups.py's corpus — config-5 columns
(year 75 values, rating 91, genre 12) plus random int group columns of 8, 100, 4000, 12 000 and 100 000 values (`g8` .. `g100k`) and a unique one (`uid`).
Two runs, because a kernel trace slows the host:

    python tools/bench_group_members.py --out calls.json                                      # time per call, profiler off
    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/bench_group_members.py
    python tools/bench_group_members.py --summarize trace/<host>/<pid>_kernel_trace.csv calls.json

Cases: one page (offset 0, limit 20, order by `rating`, ascending) grouped by each of the six columns under `rating >= 1.0` (every document),
`year >= 2000 AND rating > 7.0` (11 %) and `year = 1987 AND rating >= 1.0` (1.3 %), each with per_group 1, 3 and 16; and the contention case, a page of ONE
group (limit 1) of g8 under the 100 % filter: an eighth of the corpus enters one row's slots.

Every repetition starts a new mask epoch (restore_documents) and makes three calls: list_group_members twice (the first builds its mask in front, "cold",
the second finds it, "cached") and list_groups with the same request, whose k_group_sizes and k_group_heads are the yardsticks of k_group_members in the same
trace — the new walk reads what k_group_sizes reads, plus the order codes of the hits.  The first repetition of a case is left out; medians.  COST_DOCS
overrides the corpus size."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_list_groups import ALL, FILTERS, GROUPS, ONE, ORDER, LIST_KERNELS      # noqa: E402 (the corpus and the filters are that tool's)

DOCS = int(os.environ.get("COST_DOCS", "10000000"))
REPS = 4
PER_GROUP = (1, 3, 16)
KERNELS = ("k_filter_mask_multi", "k_group_heads_mask", "k_group_heads", "k_group_page", "k_group_sizes", "k_group_member_rows", "k_group_members") + LIST_KERNELS


def cases():
    """name -> (filter, group column, per_group, limit)"""
    out = {}
    for g, _, _ in GROUPS:
        for fname, x in FILTERS:
            for per in PER_GROUP:
                out["%s, %s, %d per group" % (g, fname, per)] = (x, g, per, 20)
    for per in PER_GROUP:
        out["g8, 100 %%, ONE group, %d per group" % per] = (ALL, "g8", per, 1)
    return out


def kernel_of(name):
    for k in KERNELS:                                                  # (k_group_heads_mask before k_group_heads, k_group_member_rows before k_group_members)
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
    # one call of this tool: [k_filter_mask_multi] k_group_heads ... (a single spec per call)
    calls, prev = [], None
    for _, k, d in rows:
        if k == "k_filter_mask_multi" or (k == "k_group_heads" and prev != "k_filter_mask_multi"):
            calls.append({})
        if calls:
            calls[-1].setdefault(k, []).append(d)
        prev = k
    warm = 1                                                           # the call that builds the order column's sort rank
    want = warm + 3 * REPS * len(cases())
    assert len(calls) == want, "the trace does not hold the launches of one run of this tool (%d calls, %d expected)" % (len(calls), want)
    host = json.load(open(calls_path)) if calls_path else {}
    print("| case | members of the set | groups | members on the page | k_group_members (us) | k_group_sizes, same request (us) | members / sizes | k_group_heads (us) | members / heads "
          "| k_group_member_rows (us) | all kernels, list_group_members cached (us) | all kernels, list_groups cached (us) | list_group_members call, cached / cold (ms) "
          "| list_groups call, cached (ms) |")
    print("|" + "---|" * 14)
    at = warm
    for name in cases():
        seg = calls[at:at + 3 * REPS]; at += 3 * REPS
        cold, cached, groups = seg[3::3], seg[4::3], seg[5::3]        # (the first repetition left out)
        assert all("k_filter_mask_multi" in c and "k_group_members" in c for c in cold), name
        assert all("k_filter_mask_multi" not in c and "k_group_members" in c and "k_group_sizes" not in c for c in cached), name
        assert all("k_group_sizes" in c and "k_group_members" not in c for c in groups), name
        med = lambda cs, k: float(np.median([sum(c.get(k, [0.0])) for c in cs]))
        walk, rows_k = med(cold + cached, "k_group_members"), med(cold + cached, "k_group_member_rows")
        sizes, heads = med(groups, "k_group_sizes"), med(cold + cached + groups, "k_group_heads")
        total = lambda cs: float(np.median([sum(sum(v) for v in c.values()) for c in cs]))
        h = host.get(name, {})
        head = "| %s | %s | %s | %s " % (name, h.get("members", "-"), h.get("groups", "-"), h.get("listed", "-"))
        tail = "| %.3f / %.3f | %.3f |" % (h["cached"], h["cold"], h["groups_cached"]) if h else "| - | - |"
        print(head + "| %.1f | %.1f | %.2f | %.1f | %.2f | %.1f | %.1f | %.1f " % (walk, sizes, walk / sizes, heads, walk / heads, rows_k, total(cached), total(groups)) + tail)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
        sys.exit(0)
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    from infidex_amd import SearchEngine, GroupMembersRequest, GroupListRequest
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
    for g, card, _ in GROUPS:
        cols[g] = rng.integers(0, card, DOCS).astype(np.int64) if card else rng.permutation(DOCS).astype(np.int64)
        e.set_column(g, cols[g], facetable=False)
    print("built in %.1f s" % (time.time() - t0), flush=True)
    t = time.perf_counter()
    first = e.list_groups(None, "g8", ORDER, True, 0, 20)             # the sort rank is built on first use: outside the timed calls
    print("first use of %s: %.1f ms; %d groups of %d documents" % (ORDER, (time.perf_counter() - t) * 1e3, first.total_groups, first.total), flush=True)
    calls = {}
    for name, (x, g, per, limit) in cases().items():
        req, greq = [GroupMembersRequest(x, g, ORDER, True, per, 0, limit)], [GroupListRequest(x, g, ORDER, True, 0, limit)]
        cold, cached, groups = [], [], []
        for rep in range(REPS):
            e.restore_documents()                                      # a new mask epoch
            t = time.perf_counter(); a = e.list_group_members(req); cold.append(time.perf_counter() - t)
            assert e.last_group_members_stats()[:3] == (1, 0, 1) and e.last_group_members_stats()[4] == 1
            t = time.perf_counter(); b = e.list_group_members(req); cached.append(time.perf_counter() - t)
            assert e.last_group_members_stats()[:3] == (0, 1, 1) and repr(a) == repr(b) and a[0].error is None
            t = time.perf_counter(); c = e.list_groups(greq); groups.append(time.perf_counter() - t)
            assert e.last_group_list_stats()[:3] == (0, 1, 1)
            assert ([m.document_ids[0] for m in a[0].groups], [m.size for m in a[0].groups], a[0].total_groups, a[0].total) == (c[0].document_ids, c[0].group_sizes, c[0].total_groups, c[0].total)
        ms = lambda v: float(np.median(v[1:])) * 1e3
        calls[name] = {"cold": ms(cold), "cached": ms(cached), "groups_cached": ms(groups), "members": a[0].total, "groups": a[0].total_groups,
                       "listed": sum(m.size for m in a[0].groups)}
        print("PHASE %s: %d members, %d groups, %d on the page; cached %.3f ms, cold %.3f ms; list_groups cached %.3f ms"
              % (name, a[0].total, a[0].total_groups, calls[name]["listed"], calls[name]["cached"], calls[name]["cold"], calls[name]["groups_cached"]), flush=True)
    if out_path:                                                       # profiler-off run only: the answer, once, against the columns
        sel = np.nonzero((year == 1987) & (rating >= 1.0))[0]
        got = e.list_group_members(ONE, "g8", None, True, 16, 0, 20)   # index order: a group's members are its sixteen lowest indices of the set
        assert got.total == len(sel) and got.total_groups == 8 and sum(m.size for m in got.groups) == len(sel), (got.total, len(sel))
        for m in got.groups:
            assert m.document_ids == [int(d) for d in sel[cols["g8"][sel] == int(m.group_value)][:16]], m.group_value
        print("members, totals and sizes equal the columns'", flush=True)
        json.dump(calls, open(out_path, "w"), indent=1)
