// Host model of field_distinct's arithmetic: infidex_amd/csrc/distinct_set.h, UNCHANGED.  The bitmap addresses are held to a plain bit array per pair, the
// capacity rule to its definition, the probe sequence to a walk written out here, and ds_insert — on a plain array, the device's load and compare-and-swap
// replaced by plain reads and writes — to std::set.  tests/test_distinct_model.py compiles and runs it under the sanitizers.
//   distinct_model         runs every case, prints "OK <addresses> <capacities> <probes> <inserts> <longest chain> <overflows>" or the first mismatch (exit 1)
#define DS_FN static inline
#include "distinct_set.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

typedef unsigned long long u64;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static u64 rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static u64 g_addr = 0, g_caps = 0, g_probes = 0, g_inserts = 0, g_chain = 0, g_overflows = 0;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); return false; } } while (0)

// every pair of G x V has a bit of its own, inside its row, inside the bitmap; the pair index is row-major
static bool addresses(uint32_t G, uint32_t V) {
    const uint32_t row = ds_row_words(V);
    CHECK((u64)row * 32 >= V && (row == 0 || (u64)(row - 1) * 32 < V), "row stride of %u values: %u words", V, row);
    CHECK(ds_bitmap_words(G, V) == (u64)G * row, "bitmap words of %u x %u", G, V);
    std::vector<uint32_t> bits((size_t)G * row, 0u);          // (heap block of exactly the bitmap's size: an address outside it is the sanitizer's)
    u64 pair = 0;
    for (uint32_t g = 0; g < G; g++) for (uint32_t v = 0; v < V; v++, pair++) {
        const uint32_t w = ds_word(g, row, v), b = ds_bit(v);
        CHECK(w >= g * row && w < (g + 1) * row, "pair (%u, %u) of %u x %u: word %u outside its row", g, v, G, V, w);
        CHECK(b && !(b & (b - 1)) && w == g * row + v / 32 && b == 1u << (v % 32), "pair (%u, %u): word %u bit %08x", g, v, w, b);
        CHECK(!(bits[w] & b), "pair (%u, %u) of %u x %u shares its bit", g, v, G, V);
        bits[w] |= b;
        CHECK(ds_pair(g, V, v) == pair && ds_key(g, V, v) == pair + 1, "pair index of (%u, %u) in %u x %u", g, v, G, V);
        g_addr++;
    }
    u64 set = 0; for (uint32_t x : bits) set += (u64)__builtin_popcount(x);
    CHECK(set == (u64)G * V, "%u x %u: %llu bits for %llu pairs", G, V, set, (u64)G * V);
    return true;
}
static bool fits() {
    CHECK(ds_bitmap_fits(1, 0xFFFFFFFFu) && ds_bitmap_fits(4096, 1u << 20) && !ds_bitmap_fits(4096, (1u << 20) + 1) && !ds_bitmap_fits(2, 0xFFFFFFFFu), "the 2^32-bit limit");
    CHECK(ds_bitmap_fits(4096, 1) && ds_bitmap_words(4096, 1) == 4096 && ds_bitmap_fits(0, 0), "small bitmaps");
    CHECK(ds_pair(4095, 0x7FFFFFFFu, 0x7FFFFFFEu) == 4095ull * 0x7FFFFFFFull + 0x7FFFFFFEull, "the pair index is 64-bit");
    return true;
}
static bool capacities() {
    const u64 pairs[] = {0, 1, 2, 7, 511, 512, 513, 1023, 1024, 4099, 8192, 8193, 65535, 65536, 65537, 10000000, (1ull << 31) - 1, 1ull << 31};
    for (u64 p : pairs) for (int d = -1; d <= 1; d++) {
        const u64 q = p + (u64)d; if (q > (1ull << 31)) continue;
        const u64 c = ds_capacity(q);
        CHECK(c >= DS_MIN_CAPACITY && !(c & (c - 1)) && c >= 2 * q && (c == DS_MIN_CAPACITY || c / 2 < 2 * q), "capacity of %llu pairs: %llu", q, c);
        g_caps++;
    }
    CHECK(ds_capacity(4099) == 16384 && ds_capacity(4096) == 8192 && ds_capacity(0) == DS_MIN_CAPACITY && ds_capacity(1ull << 31) == 1ull << 32, "capacity examples");
    CHECK(ds_max_pairs(4099, 7, 4099) == 4099 && ds_max_pairs(4099, 1, 7) == 7 && ds_max_pairs(10000000, 4096, 0x7FFFFFFFu) == 10000000 && ds_max_pairs(5, 0, 9) == 0, "the pairs that can occur");
    return true;
}
// the probe sequence of a key: capacity distinct slots, consecutive modulo the capacity, from the hash's low bits — wrap-around included
static bool probes(u64 cap, u64 key) {
    std::vector<char> seen(cap, 0);
    const u64 first = ds_hash(key) & (cap - 1);
    for (u64 i = 0; i < cap; i++) {
        const u64 s = ds_slot(key, cap, i);
        CHECK(s < cap && s == (first + i) % cap && !seen[s], "probe %llu of key %llu in %llu slots: slot %llu", i, key, cap, s);
        seen[s] = 1; g_probes++;
    }
    return true;
}
// ds_insert on a plain table; *visited the slots it read
static int insert(std::vector<u64>& tab, u64 key, u64* visited) {
    u64 reads = 0;
    const int r = ds_insert((u64)tab.size(), key, [&](u64 slot) { reads++; return (u64)tab.at(slot); },
                            [&](u64 slot, u64 k) { const u64 old = tab.at(slot); if (old == 0) tab.at(slot) = k; return old; });
    if (visited) *visited = reads;
    return r;
}
// keys (with repeats) into a table of cap slots: new exactly once per key, seen afterwards, the table's keys = std::set's, no key twice
static bool inserts(u64 cap, const std::vector<u64>& keys, const char* what) {
    std::vector<u64> tab(cap, 0); std::set<u64> ref;
    for (u64 k : keys) {
        u64 visited = 0;
        const int r = insert(tab, k, &visited);
        const bool fresh = ref.insert(k).second;
        CHECK(r == (fresh ? DS_NEW : DS_SEEN), "%s: key %llu: %d, std::set says %s", what, k, r, fresh ? "new" : "seen");
        CHECK(visited >= 1 && visited <= ref.size(), "%s: key %llu visited %llu slots with %zu keys in the table", what, k, visited, ref.size());
        if (visited > g_chain) g_chain = visited;
        g_inserts++;
    }
    std::multiset<u64> in; for (u64 x : tab) if (x) in.insert(x);
    CHECK(in.size() == ref.size() && std::set<u64>(in.begin(), in.end()) == ref, "%s: the table holds %zu keys, std::set %zu", what, in.size(), ref.size());
    for (u64 k : ref) CHECK(insert(tab, k, nullptr) == DS_SEEN, "%s: key %llu is not found again", what, k);
    return true;
}
// keys whose probe sequences all begin at `slot` of a table of cap slots
static std::vector<u64> colliding(u64 cap, u64 slot, size_t n) {
    std::vector<u64> out;
    for (u64 k = 1; out.size() < n; k++) if ((ds_hash(k) & (cap - 1)) == slot) out.push_back(k);
    return out;
}
// A deliberately undersized table (host only: the device's is sized never to fill): cap keys fill it, every further key visits all cap slots and reports
// the overflow; the table is unchanged and the keys in it are still found.
static bool overflow(u64 cap) {
    std::vector<u64> tab(cap, 0); std::set<u64> ref;
    for (u64 k = 1; ref.size() < cap; k += 3) { CHECK(insert(tab, k, nullptr) == DS_NEW, "filling %llu slots: key %llu", cap, k); ref.insert(k); }
    const std::vector<u64> full = tab;
    for (u64 k = 2; k < 2 + 3 * 40; k += 3) {
        u64 visited = 0;
        CHECK(insert(tab, k, &visited) == DS_OVERFLOW && visited == cap, "a full table of %llu slots: key %llu visited %llu", cap, k, visited);
        g_overflows++;
    }
    CHECK(tab == full, "a full table of %llu slots changed", cap);
    for (u64 k : ref) CHECK(insert(tab, k, nullptr) == DS_SEEN, "a full table of %llu slots: key %llu", cap, k);
    return true;
}

int main() {
    const uint32_t Gs[] = {1, 2, 7, 33}, Vs[] = {1, 7, 31, 32, 33, 63, 64, 65, 100, 3000, 4099};
    for (uint32_t G : Gs) for (uint32_t V : Vs) if (!addresses(G, V)) return 1;
    if (!addresses(4096, 7) || !addresses(3000, 129) || !fits() || !capacities()) return 1;
    for (u64 cap : {(u64)DS_MIN_CAPACITY, 8192ull, 16384ull}) {
        for (int i = 0; i < 24; i++) if (!probes(cap, 1 + rnd() % (1ull << 43))) return 1;
        // keys whose sequence starts at the table's last slots: the wrap-around
        for (u64 back = 1; back <= 3; back++) for (u64 k : colliding(cap, cap - back, 2)) if (!probes(cap, k)) return 1;
    }
    // the GPU tests' two shapes: 4 099 members into 7 pairs and into 4 099 pairs, in the table the capacity rule gives them
    for (int round = 0; round < 4; round++) {
        std::vector<u64> seven, all, mixed;
        for (int i = 0; i < 4099; i++) { seven.push_back(ds_key(0, 7, (uint32_t)(rnd() % 7))); all.push_back(ds_key(0, 4099, (uint32_t)i)); mixed.push_back(ds_key((uint32_t)(rnd() % 7), 4099, (uint32_t)(rnd() % 4099))); }
        if (!inserts(ds_capacity(ds_max_pairs(4099, 1, 7)), seven, "7 pairs") || !inserts(ds_capacity(ds_max_pairs(4099, 1, 4099)), all, "4099 pairs") ||
            !inserts(ds_capacity(ds_max_pairs(4099, 7, 4099)), mixed, "7 x 4099 pairs")) return 1;
        std::vector<u64> wide; for (int i = 0; i < 20000; i++) wide.push_back(1 + rnd() % (1ull << 43));
        if (!inserts(ds_capacity(20000), wide, "random 43-bit keys")) return 1;
    }
    // a full chain of collisions: 512 keys that all hash to one slot — at the table's start, and at its last slot, where the chain wraps — each repeated
    for (u64 slot : {0ull, DS_MIN_CAPACITY - 1, DS_MIN_CAPACITY - 200}) {
        std::vector<u64> chain = colliding(DS_MIN_CAPACITY, slot, 512), twice = chain;
        twice.insert(twice.end(), chain.rbegin(), chain.rend());
        const u64 before = g_chain;
        g_chain = 0;
        if (!inserts(DS_MIN_CAPACITY, twice, "one chain")) return 1;
        if (g_chain != 512) { printf("FAIL a chain of 512 colliding keys: longest walk %llu\n", g_chain); return 1; }
        if (before > g_chain) g_chain = before;
    }
    for (u64 cap : {1ull, 2ull, 8ull, 64ull, 1024ull}) if (!overflow(cap)) return 1;
    printf("OK %llu %llu %llu %llu %llu %llu\n", g_addr, g_caps, g_probes, g_inserts, g_chain, g_overflows);
    return 0;
}
