// Host model of list_documents' selection: infidex_amd/csrc/listing_select.h, UNCHANGED, driven serially the way the kernels drive it
// (histogram -> pick -> ... -> thresholds -> classes -> slots -> sort of the page) over generated masked key arrays, and compared element for
// element with a plain sort of (key, document).  tests/test_listing_model.py compiles and runs it.
//   listing_model            runs every case, prints "OK <selects> <pages compared>" or the first mismatch (exit 1)
#define LS_FN static inline
#include "listing_select.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

typedef unsigned long long u64;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }

static std::set<std::tuple<uint32_t, uint32_t, uint32_t>> g_parted;      // (digit bits, passes, pass after which lo and hi differ; passes = never)

// the device's walk, serially: keys[d] (ascending keys, 1 .. nvals), member[d]; returns false on an inconsistency of its own
static bool select_page(const std::vector<uint32_t>& keys, const std::vector<uint8_t>& member, uint32_t nvals, bool asc, uint32_t db, uint32_t offset, uint32_t limit,
                        std::vector<u64>& page, uint32_t& total) {
    const uint32_t n = (uint32_t)keys.size(), nb = 1u << db, passes = ls_passes(nvals, db);
    ls_target t[2] = {{0, 0}, {0, 0}};
    uint32_t last = 0; total = 0; page.clear();
    uint32_t parted = passes;
    std::vector<uint32_t> hist(2 * (size_t)nb);
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = ls_shift(p, passes, db);
        std::fill(hist.begin(), hist.end(), 0u);
        for (uint32_t d = 0; d < n; d++) {                                   // k_list_hist
            if (!member[d]) continue;
            const uint32_t k = ls_mirror(keys[d], nvals, asc), dg = ls_digit(k, shift, db);
            for (int x = 0; x < 2; x++) if (ls_under_prefix(k, t[x].prefix, shift, db)) hist[(size_t)x * nb + dg]++;
        }
        if (p == 0) {                                                        // k_list_pick
            for (uint32_t b = 0; b < nb; b++) total += hist[b];
            if (offset >= total) return true;
            last = (uint32_t)std::min<u64>((u64)offset + limit, total) - 1u;
            t[0].resid = offset; t[1].resid = last;
        }
        for (int x = 0; x < 2; x++) {
            uint32_t dg = 0, rest = 0;
            if (!ls_pick(hist.data() + (size_t)x * nb, nb, t[x].resid, &dg, &rest)) { printf("FAIL pick found no bin\n"); return false; }
            t[x].prefix = ls_extend(t[x].prefix, dg, db); t[x].resid = rest;
        }
        if (parted == passes && t[0].prefix != t[1].prefix) parted = p;
    }
    g_parted.insert(std::make_tuple(db, passes, parted));
    const ls_page P = ls_make_page(t[0], t[1], offset, last);
    uint32_t cls[3] = {0, 0, 0};
    for (uint32_t d = 0; d < n; d++) if (member[d]) { const uint32_t c = ls_class(P, ls_mirror(keys[d], nvals, asc)); if (c) cls[c - 1]++; }      // k_list_count + k_list_prefix
    std::vector<u64> slots(P.count, ~0ull); uint32_t idx[3] = {0, 0, 0}, written = 0;
    for (uint32_t d = 0; d < n; d++) {                                       // k_list_gather
        if (!member[d]) continue;
        const uint32_t k = ls_mirror(keys[d], nvals, asc), c = ls_class(P, k);
        if (!c) continue;
        const uint32_t s = ls_slot(P, c, idx[c - 1]++, cls[0]);
        if (s == LS_NONE) continue;
        if (s >= P.count || slots[s] != ~0ull) { printf("FAIL slot %u of %u written twice or out of range\n", s, P.count); return false; }
        slots[s] = ((u64)k << 32) | d; written++;
    }
    if (written != P.count) { printf("FAIL %u of %u slots written\n", written, P.count); return false; }
    std::sort(slots.begin(), slots.end());                                   // k_list_sort
    page = slots;
    return true;
}

static u64 g_selects = 0, g_pages = 0;
static bool check(const std::vector<uint32_t>& keys, const std::vector<uint8_t>& member, uint32_t nvals, uint32_t db, const char* what) {
    for (int dir = 0; dir < 2; dir++) {
        const bool asc = dir == 0;
        std::vector<u64> ref;
        for (uint32_t d = 0; d < keys.size(); d++) if (member[d]) ref.push_back(((u64)ls_mirror(keys[d], nvals, asc) << 32) | d);
        std::sort(ref.begin(), ref.end());
        const uint32_t total = (uint32_t)ref.size();
        // the longest run of equal keys in the order: offsets at its first element, inside it and at its last
        uint32_t a = 0, b = 0;
        for (uint32_t i = 0; i < total;) { uint32_t j = i; while (j + 1 < total && (ref[j + 1] >> 32) == (ref[i] >> 32)) j++; if (j - i > b - a) { a = i; b = j; } i = j + 1; }
        std::vector<uint32_t> offs = {0u, a, (a + b) / 2, b, total ? total - 1 : 0u, total, total + 5, total / 3, 0x7FFFFFFFu};
        const uint32_t limits[] = {1u, 1024u, 97u};
        for (uint32_t off : offs) for (uint32_t lim : limits) {
            std::vector<u64> page; uint32_t tot = 0;
            if (!select_page(keys, member, nvals, asc, db, off, lim, page, tot)) { printf("  in %s db %u nvals %u asc %d offset %u limit %u\n", what, db, nvals, (int)asc, off, lim); return false; }
            g_selects++;
            const uint32_t lo = std::min(off, total), hi = (uint32_t)std::min<u64>((u64)off + lim, total);
            bool ok = tot == total && page.size() == hi - lo;
            for (uint32_t i = 0; ok && i < hi - lo; i++) ok = page[i] == ref[lo + i];
            if (!ok) { printf("FAIL %s db %u nvals %u asc %d offset %u limit %u: total %u (want %u), %zu rows (want %u)\n", what, db, nvals, (int)asc, off, lim, tot, total, page.size(), hi - lo); return false; }
            g_pages++;
        }
    }
    return true;
}

int main() {
    const uint32_t N = 2600;
    const uint32_t dbs[] = {4u, 5u, 11u};
    for (uint32_t db : dbs) for (uint32_t B = 1; B <= 32; B++) {
        const uint32_t nvals = B == 32 ? 0xFFFFFFFEu : (1u << B) - 2u;      // bits(nvals + 1) == B; keys reach 2^B - 2
        if (ls_key_bits(nvals) != B) { printf("FAIL key bits of %u: %u\n", nvals, ls_key_bits(nvals)); return 1; }
        std::vector<uint8_t> member(N), none(N, 0);
        for (auto& m : member) m = rnd() % 5 < 3;
        std::vector<uint32_t> keys(N, 1);
        if (nvals == 0) {                                                    // B = 1: no value, hence no member
            if (!check(keys, none, nvals, db, "no values")) return 1;
            continue;
        }
        if (!check(keys, none, nvals, db, "empty set")) return 1;
        for (auto& k : keys) k = nvals;                                      // all keys equal (the largest)
        if (!check(keys, member, nvals, db, "all equal")) return 1;
        {                                                                    // all keys distinct, the extremes among them
            const uint32_t m = (uint32_t)std::min<u64>(N, nvals);
            std::set<uint32_t> seen = {1u, nvals};
            while (seen.size() < m) seen.insert(1u + (uint32_t)(((u64)rnd() << 16 ^ rnd()) % nvals));
            std::vector<uint32_t> v(seen.begin(), seen.end());
            for (uint32_t i = (uint32_t)v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd() % i]);
            std::vector<uint32_t> kd(m); std::vector<uint8_t> md(m);
            for (uint32_t i = 0; i < m; i++) { kd[i] = v[i]; md[i] = rnd() % 7 != 0; }
            if (!check(kd, md, nvals, db, "all distinct")) return 1;
        }
        // two heavy keys that share every digit above pass p and differ in it, random keys around them: lo and hi part at pass p for the pages that span both
        const uint32_t passes = ls_passes(nvals, db);
        for (uint32_t p = 0; p < passes; p++) {
            const uint32_t shift = ls_shift(p, passes, db);
            uint32_t A = 1u + (uint32_t)(((u64)rnd() << 16 ^ rnd()) % nvals);
            uint32_t Bk = (uint32_t)(((u64)A ^ (1ull << shift)));
            if (Bk < 1 || Bk > nvals) { A = 1; Bk = (uint32_t)(1ull ^ (1ull << shift)); }
            if (Bk < 1 || Bk > nvals) continue;                              // (only the top digit of a narrow key range)
            for (uint32_t d = 0; d < N; d++) { const uint32_t r = rnd() % 10; keys[d] = r < 4 ? A : r < 8 ? Bk : 1u + (uint32_t)(((u64)rnd() << 16 ^ rnd()) % nvals); }
            if (!check(keys, member, nvals, db, "two heavy keys")) return 1;
            // ... and the same two keys alone: every page that holds both parts exactly at pass p
            for (uint32_t d = 0; d < N; d++) keys[d] = rnd() & 1 ? A : Bk;
            if (!check(keys, member, nvals, db, "two keys")) return 1;
        }
        for (uint32_t d = 0; d < N; d++) keys[d] = 1u + (uint32_t)(((u64)rnd() << 16 ^ rnd()) % std::min(nvals, 37u));      // many ties at the low end
        if (!check(keys, member, nvals, db, "ties")) return 1;
    }
    // lo and hi parted at every possible pass, and never (a page inside one key), for every pass count that was walked
    std::set<std::pair<uint32_t, uint32_t>> shapes;
    for (auto& x : g_parted) shapes.insert({std::get<0>(x), std::get<1>(x)});
    uint32_t maxPasses11 = 0, maxPasses4 = 0;
    for (auto& s : shapes) {
        for (uint32_t p = 0; p <= s.second; p++)
            if (!g_parted.count(std::make_tuple(s.first, s.second, p))) { printf("FAIL digit bits %u, %u passes: lo and hi never parted at pass %u\n", s.first, s.second, p); return 1; }
        if (s.first == 11) maxPasses11 = std::max(maxPasses11, s.second);
        if (s.first == 4) maxPasses4 = std::max(maxPasses4, s.second);
    }
    if (maxPasses11 != 3 || maxPasses4 != 8) { printf("FAIL pass counts walked: %u at 11 bits, %u at 4 bits\n", maxPasses11, maxPasses4); return 1; }
    printf("OK %llu %llu\n", g_selects, g_pages);
    return 0;
}
