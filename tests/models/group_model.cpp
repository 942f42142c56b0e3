// Host model of list_groups' per-member arithmetic: infidex_amd/csrc/group_heads.h, UNCHANGED.  The lookup of a group code among a page's sorted codes is
// held to a linear scan, the composite to a comparison of (key, document) pairs.  tests/test_group_model.py compiles and runs it.
//   group_model            runs every case, prints "OK <code lists> <lookups> <composite pairs>" or the first mismatch (exit 1)
#define GH_FN static inline
#include "group_heads.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

typedef unsigned long long u64;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }

static u64 g_lists = 0, g_lookups = 0, g_pairs = 0;
static uint32_t g_maxReads = 0;

// the reads of one lookup: gh_find's loop, re-walked, and the final comparison
static uint32_t reads_of(uint32_t n) { uint32_t c = 0; for (uint32_t s = gh_first_step(n); s; s >>= 1) c++; return c; }

static uint32_t linear_find(const std::vector<uint32_t>& codes, uint32_t code) {
    for (uint32_t i = 0; i < codes.size(); i++) if (codes[i] == code) return i;
    return GH_NONE;
}
static bool look(const std::vector<uint32_t>& codes, uint32_t code, const char* what) {
    const uint32_t got = gh_find(codes.data(), (uint32_t)codes.size(), code), lin = linear_find(codes, code);
    g_lookups++;
    if (got == lin) return true;
    printf("FAIL %s: code %u among %zu codes: position %u, linear scan %u\n", what, code, codes.size(), got, lin);
    return false;
}
// every code of the list, its neighbours, and codes at and beyond both ends
static bool walk(const std::vector<uint32_t>& codes, const char* what) {
    for (size_t i = 1; i < codes.size(); i++) if (codes[i] <= codes[i - 1]) { printf("FAIL %s: the case's own codes are not ascending and distinct\n", what); return false; }
    for (uint32_t c : codes) if (!look(codes, c, what) || !look(codes, c + 1u, what) || !look(codes, c - 1u, what)) return false;
    const uint32_t ends[] = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu, codes.empty() ? 5u : codes.front(), codes.empty() ? 5u : codes.back()};
    for (uint32_t c : ends) if (!look(codes, c, what)) return false;
    for (int i = 0; i < 64; i++) if (!look(codes, rnd(), what)) return false;
    if (!codes.empty()) g_maxReads = std::max(g_maxReads, reads_of((uint32_t)codes.size()));
    g_lists++;
    return true;
}

int main() {
    const uint32_t sizes[] = {0, 1, 2, 3, 7, 8, 9, 511, 512, 513, 1023, 1024};
    for (uint32_t n : sizes) {
        std::vector<uint32_t> c(n);
        for (uint32_t i = 0; i < n; i++) c[i] = i;                                         // from code 0: nothing below
        if (!walk(c, "dense from zero")) return 1;
        for (uint32_t i = 0; i < n; i++) c[i] = 0xFFFFFFFFu - (n - 1 - i);                 // up to the largest code: nothing above
        if (!walk(c, "dense to the top")) return 1;
        for (uint32_t i = 0; i < n; i++) c[i] = 1000u + 3u * i;                            // gaps between all neighbours, room at both ends
        if (!walk(c, "every third")) return 1;
        for (int rep = 0; rep < 8; rep++) {
            std::set<uint32_t> s;
            const uint32_t span = rep < 4 ? 4u * n + 8u : 0xFFFFFFFFu;                     // crowded, then spread over all codes
            while (s.size() < n) s.insert(rnd() % span);
            c.assign(s.begin(), s.end());
            if (!walk(c, "random")) return 1;
        }
    }
    if (g_maxReads != 11) { printf("FAIL the widest lookup read %u codes, 11 expected\n", g_maxReads); return 1; }
    // composites order as (key, document) pairs do, the low word is the document, none is the empty entry
    for (int i = 0; i < 200000; i++) {
        const uint32_t bits = 1 + rnd() % 32;
        const uint32_t ka = 1u + rnd() % (bits == 32 ? 0xFFFFFFFFu : (1u << bits)), kb = (i & 3) ? 1u + rnd() % (bits == 32 ? 0xFFFFFFFFu : (1u << bits)) : ka;
        const uint32_t da = rnd() & 0x7FFFFFFFu, db = (i & 4) ? rnd() & 0x7FFFFFFFu : da;
        const u64 a = gh_composite(ka, da), b = gh_composite(kb, db);
        const bool lessPair = ka != kb ? ka < kb : da < db;
        if ((a < b) != lessPair || (a == b) != (ka == kb && da == db) || gh_head(a) != da || a == GH_EMPTY) { printf("FAIL composite (%u, %u) against (%u, %u)\n", ka, da, kb, db); return 1; }
        if (!gh_is_head(a, da) || gh_is_head(GH_EMPTY, da) || (da != db && gh_is_head(a, db))) { printf("FAIL head of (%u, %u)\n", ka, da); return 1; }
        g_pairs++;
    }
    if (gh_composite(0xFFFFFFFFu, 0x7FFFFFFFu) == GH_EMPTY || gh_composite(1u, 0u) != (1ull << 32)) { printf("FAIL the composite's ends\n"); return 1; }
    printf("OK %llu %llu %llu\n", g_lists, g_lookups, g_pairs);
    return 0;
}
