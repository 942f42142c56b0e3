// The lowering of a filter leaf over a LIST column (infidex_amd/csrc/host/list_columns.h over host/filter.h, both unchanged) without a GPU.
// For int, double and string element dictionaries and each of the 13 LeafOps: the elements are encoded with encode_column, every leaf gets its bitmap over
// the element dictionary (list_leaf_table) and its empty-list bit, the K bitmaps are laid side by side (list_leaf_maps) and a loop that does what k_list_leaf
// does — one hit word per element, ORed into its document — gives the derived bit of every document.  That bit must equal the OR of leaf_holds() over the
// document's elements taken as scalar values, and leaf_holds() of a null value for an empty list; list_leaf_bit() must agree too.
// Output: one line per (kind, operator): "<kind> <op> <documents> <bits set> <empty-list bit> <mismatches>".  Exit status 1 on any mismatch.
#include "../../infidex_amd/csrc/host/list_columns.h"
#include <cstdio>

using namespace infx::filt;

static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static std::vector<Boxed> pool_of(int kind) {
    std::vector<Boxed> p;
    if (kind == 1) {
        for (long long v = -5; v < 70; v++) { Boxed b; b.kind = 1; b.i = v; p.push_back(b); }
        for (long long v : {1000000007LL, -9000000000000000000LL, 9007199254740993LL}) { Boxed b; b.kind = 1; b.i = v; p.push_back(b); }
    } else if (kind == 2) {
        const double xs[] = {0.0, -0.0, 1.0, 2.5, -2.5, 10.0, 9.0, 1e15, 1e-5, 12.25, NAN, INFINITY, -INFINITY, 0.1, 100.0, 33.0, 7.0, 1234.5};
        for (double x : xs) { Boxed b; b.kind = 2; b.d = x; p.push_back(b); }
        for (int i = 0; i < 40; i++) { Boxed b; b.kind = 2; b.d = 3.0 + i * 0.5; p.push_back(b); }
    } else {
        const char* xs[] = {"", "sale", "Sale", "SALE", "new", "10", "9", "9.5", "abc", "a%c", "abd", "\xC7\x86ungla", "\xC7\x84ungla", "x y", "sal", "resale", "salesman", "1,000", " 12 ", "NaN"};
        for (const char* x : xs) { Boxed b; b.kind = 3; b.s = x; p.push_back(b); }
        for (int i = 0; i < 30; i++) { Boxed b; b.kind = 3; b.s = "tag" + std::to_string(i); p.push_back(b); }
    }
    return p;
}
static std::vector<Leaf> leaves_of(int kind) {
    const std::string a = kind == 3 ? "sale" : "10", lo = kind == 3 ? "abc" : "2.5", hi = kind == 3 ? "sal" : "33";
    return {
        {"f", L_EQ, {a}}, {"f", L_GT, {a}}, {"f", L_GE, {a}}, {"f", L_LT, {a}}, {"f", L_LE, {a}}, {"f", L_BETWEEN, {lo, hi}},
        {"f", L_IN, {a, "9", "NEW", "-0"}}, {"f", L_CONTAINS, {kind == 3 ? "ale" : "5"}}, {"f", L_STARTS, {kind == 3 ? "SAL" : "1"}},
        {"f", L_ENDS, {kind == 3 ? "le" : "5"}}, {"f", L_LIKE, {kind == 3 ? "_a%" : "1%"}}, {"f", L_ISNULL, {}}, {"f", L_NOTNULL, {}},
    };
}

int main() {
    int bad = 0;
    for (int kind = 1; kind <= 3; kind++) {
        const std::vector<Boxed> pool = pool_of(kind);
        // the lists: empty ones at both ends and in a run, lengths 1, 2, 5, 33 and 70, a list of one repeated value; which elements: a fixed generator
        const size_t n = 211; uint64_t seed = 12345u + (uint64_t)kind;
        std::vector<std::vector<Boxed>> lists(n);
        for (size_t d = 1; d + 1 < n; d++) {
            if (d >= 40 && d < 60) continue;
            const size_t len = d == 7 ? 70 : d == 8 ? 33 : d % 6 == 0 ? 0 : d % 6 == 1 ? 1 : d % 6 == 2 ? 2 : d % 6 == 3 ? 5 : 3;
            for (size_t j = 0; j < len; j++) lists[d].push_back(d == 9 ? pool[3] : pool[lcg(seed) % pool.size()]);
        }
        for (size_t v = 0; v < pool.size(); v++) lists[100 + v % 50].push_back(pool[v]);      // every value occurs
        std::vector<Boxed> flat; ListColumn c; c.name = "f"; c.kind = kind; c.off.push_back(0);
        for (auto& l : lists) { for (auto& x : l) flat.push_back(x); c.off.push_back((uint32_t)flat.size()); }
        if (kind == 1) encode_column(c.dict, flat.size(), [&](size_t j) { return flat[j]; }, (long long)0);
        else if (kind == 2) encode_column(c.dict, flat.size(), [&](size_t j) { return flat[j]; }, (uint64_t)0);
        else encode_column(c.dict, flat.size(), [&](size_t j) { return flat[j]; }, std::string());
        const std::vector<Leaf> leaves = leaves_of(kind);
        const size_t K = leaves.size(), W = (c.dict.dict.size() + 31) / 32;
        std::vector<std::vector<uint32_t>> tables(K); uint32_t emptyBits = 0;
        for (size_t k = 0; k < K; k++) if (list_leaf_table(leaves[k], c, tables[k])) emptyBits |= 1u << k;
        std::vector<uint32_t> maps; list_leaf_maps(tables, W, maps);
        for (size_t k = 0; k < K; k++) {
            size_t set = 0; int mism = 0;
            for (size_t d = 0; d < n; d++) {
                // the device's walk: one K-bit hit word per element, ORed into the document's word; an empty list takes the empty bits
                uint32_t word = 0;
                for (uint32_t e = c.off[d]; e < c.off[d + 1]; e++) { const uint32_t v = c.dict.codes[e]; for (size_t j = 0; j < K; j++) word |= ((maps[(size_t)(v >> 5) * K + j] >> (v & 31)) & 1u) << j; }
                if (c.off[d] == c.off[d + 1]) word = emptyBits;
                const bool bit = (word >> k) & 1u;
                bool want = false;
                if (lists[d].empty()) want = leaf_holds(leaves[k], Boxed());
                else for (auto& x : lists[d]) want = want || leaf_holds(leaves[k], x);
                if (bit != want || list_leaf_bit(c, tables[k], (emptyBits >> k) & 1u, d) != want) mism++;
                set += bit;
            }
            printf("%d %d %zu %zu %u %d\n", kind, (int)leaves[k].op, n, set, (emptyBits >> k) & 1u, mism);
            bad += mism;
        }
        // two leaves never share a cache key unless they are the same leaf
        for (size_t i = 0; i < K; i++) for (size_t j = 0; j < i; j++) if (list_leaf_key(leaves[i]) == list_leaf_key(leaves[j])) { printf("KEY %zu %zu\n", i, j); bad++; }
    }
    if (list_leaf_key(Leaf{"f", L_IN, {"a:1", "b"}}) == list_leaf_key(Leaf{"f", L_IN, {"a", "1:b"}})) { printf("KEY ambiguous\n"); bad++; }
    return bad ? 1 : 0;
}
