// Host model of range_facets' per-document lookup: infidex_amd/csrc/range_buckets.h, UNCHANGED, walked for every rank 0 .. nvals of generated threshold
// sets and compared with a linear scan of the thresholds.  tests/test_range_buckets_model.py compiles and runs it.
//   range_model            runs every case, prints "OK <cases> <ranks compared>" or the first mismatch (exit 1)
#define RB_FN static inline
#include "range_buckets.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned long long u64;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }

static u64 g_cases = 0, g_ranks = 0;
static uint32_t g_maxReads = 0;

// the reads of one lookup: rb_upper_bound's loop, re-walked
static uint32_t reads_of(uint32_t n) { uint32_t c = 0; for (uint32_t s = rb_first_step(n); s; s >>= 1) c++; return c; }

// the linear scan the contract states: NaN slot below nanRanks, else the number of thresholds <= r
static uint32_t linear_slot(const std::vector<uint32_t>& thr, uint32_t nanRanks, uint32_t r) {
    if (r < nanRanks) return (uint32_t)thr.size() + 1u;
    uint32_t j = 0;
    for (uint32_t t : thr) j += t <= r ? 1u : 0u;
    return j;
}

static bool walk(const std::vector<uint32_t>& thr, uint32_t nanRanks, uint32_t nvals, const char* what) {
    const uint32_t ne = (uint32_t)thr.size();
    if (ne < RB_MIN_EDGES || ne > RB_MAX_EDGES) { printf("FAIL %s: %u edges\n", what, ne); return false; }
    for (uint32_t i = 0; i < ne; i++) if (thr[i] < nanRanks || thr[i] > nvals || (i && thr[i] < thr[i - 1])) { printf("FAIL %s: bad thresholds of the case itself\n", what); return false; }
    std::vector<u64> cnt(rb_slots(ne), 0), want(rb_slots(ne), 0);
    for (u64 r = 0; r <= nvals; r++) {                                       // rank nvals does not occur; the lookup must hold there too
        const uint32_t got = rb_slot(thr.data(), ne, nanRanks, (uint32_t)r), lin = linear_slot(thr, nanRanks, (uint32_t)r);
        if (got != lin || got >= rb_slots(ne)) { printf("FAIL %s: rank %llu of %u values, %u edges, nanRanks %u: slot %u, linear scan %u\n", what, r, nvals, ne, nanRanks, got, lin); return false; }
        cnt[got]++; want[lin]++;
        g_ranks++;
    }
    // the slots partition the ranks: bucket j - 1 holds thr[j] - thr[j - 1] of them
    for (uint32_t j = 1; j < ne; j++) if (cnt[j] != (u64)thr[j] - thr[j - 1]) { printf("FAIL %s: bucket %u holds %llu ranks, thresholds say %u\n", what, j - 1, cnt[j], thr[j] - thr[j - 1]); return false; }
    if (cnt[0] != (u64)thr[0] - nanRanks || cnt[rb_nan_slot(ne)] != nanRanks || cnt[ne] != (u64)nvals + 1 - thr[ne - 1]) { printf("FAIL %s: below / nan / above\n", what); return false; }
    g_maxReads = std::max(g_maxReads, reads_of(ne));
    g_cases++;
    return true;
}

int main() {
    const uint32_t buckets[] = {1, 2, 3, 7, 8, 100, 255, 256};
    const uint32_t sizes[] = {1, 2, 3, 100, 1u << 17};
    for (uint32_t nvals : sizes)
        for (uint32_t B : buckets)
            for (uint32_t nanRanks = 0; nanRanks < 2; nanRanks++) {
                if (nanRanks > nvals) continue;
                const uint32_t ne = B + 1;
                std::vector<uint32_t> t(ne);
                // all thresholds equal: every bucket empty — at the bottom, in the middle, at the top (nothing above)
                const uint32_t levels[] = {nanRanks, nanRanks + (nvals - nanRanks) / 2, nvals};
                for (uint32_t v : levels) { std::fill(t.begin(), t.end(), v); if (!walk(t, nanRanks, nvals, "all equal")) return 1; }
                // evenly spread from thr[0] = 0 (or nanRanks: nothing below) to thr[B] = nvals (nothing above)
                for (uint32_t i = 0; i < ne; i++) t[i] = nanRanks + (uint32_t)((u64)(nvals - nanRanks) * i / B);
                if (t[0] != nanRanks || t[B] != nvals) { printf("FAIL the spread case\n"); return 1; }
                if (!walk(t, nanRanks, nvals, "spread")) return 1;
                // strictly inside: something below and something above whenever there is room
                for (uint32_t i = 0; i < ne; i++) t[i] = nanRanks + (uint32_t)((u64)(nvals - nanRanks) * (i + 1) / (ne + 1));
                if (!walk(t, nanRanks, nvals, "inside")) return 1;
                // random thresholds with runs of equal values (few distinct levels), and fully random ones
                for (int rep = 0; rep < 6; rep++) {
                    const uint32_t levelsN = rep < 3 ? 1 + rnd() % 4 : ne;
                    std::vector<uint32_t> lv(levelsN);
                    for (uint32_t& x : lv) x = nanRanks + (uint32_t)(rnd() % ((u64)nvals - nanRanks + 1));
                    for (uint32_t i = 0; i < ne; i++) t[i] = lv[rnd() % levelsN];
                    std::sort(t.begin(), t.end());
                    if (!walk(t, nanRanks, nvals, "random")) return 1;
                }
            }
    if (g_maxReads != 9) { printf("FAIL the widest lookup read %u thresholds, 9 expected\n", g_maxReads); return 1; }
    if (rb_lds_words(RB_MAX_EDGES) != 257 + 259 + 2 || rb_slots(2) != 4 || rb_nan_slot(2) != 3) { printf("FAIL the slot layout\n"); return 1; }
    printf("OK %llu %llu\n", g_cases, g_ranks);
    return 0;
}
