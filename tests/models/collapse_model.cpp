// Host model of k_collapse (infidex_amd/csrc/collapse.hip.inc): collapse.h, unchanged, walked step by step as the kernel walks it — the power-of-two bitonic
// network over row indices with pad indices, the segment starts, the two exclusive counts — and held to a brute-force fold of the list: a row is kept when
// fewer than `keep` earlier rows have its code, the first mr kept rows are returned, a row's size is the number of rows with its code.
// Prints "OK <cases>"; any difference prints the case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <random>
#include <set>
#include <vector>
#define CLP_FN static inline
#include "collapse.h"

struct Answer { std::vector<uint32_t> rows, codes, sizes; uint32_t groups = 0, ranked = 0; };

// the kernel's steps, one thread
static Answer by_steps(const std::vector<uint32_t>& code, uint32_t keep, uint32_t mr) {
    const uint32_t n = (uint32_t)code.size();
    uint32_t n2 = 2; while (n2 < n) n2 <<= 1;
    std::vector<uint16_t> idx(n2), seg(n + 1), rank(n), size(n);
    std::vector<uint8_t> flag(n);
    std::vector<uint32_t> pos(n);
    for (uint32_t i = 0; i < n2; i++) idx[i] = (uint16_t)i;
    auto less = [&](uint16_t a, uint16_t b) { return clp_before(code.data(), n, a, b); };
    if (n > 1)
        for (uint32_t k = 2; k <= n2; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1)
                for (uint32_t i = 0; i < n2; i++) {
                    const uint32_t ixj = i ^ j;
                    if (ixj > i) { const uint16_t x = idx[i], y = idx[ixj]; const bool up = (i & k) == 0; if (up ? less(y, x) : less(x, y)) { idx[i] = y; idx[ixj] = x; } }
                }
    uint32_t groups = 0;
    for (uint32_t p = 0; p < n; p++) { flag[p] = (uint8_t)clp_starts(code.data(), idx.data(), p); pos[p] = groups; groups += flag[p]; }
    for (uint32_t p = 0; p < n; p++) if (flag[p]) seg[pos[p]] = (uint16_t)p;
    seg[groups] = (uint16_t)n;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t g = clp_segment(pos[p], flag[p]), row = idx[p];
        rank[row] = (uint16_t)clp_rank(seg.data(), g, p); size[row] = (uint16_t)clp_size(seg.data(), g);
    }
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n; i++) { flag[i] = (uint8_t)clp_keeps(rank[i], keep); pos[i] = kept; kept += flag[i]; }
    const uint32_t nOut = clp_returned(kept, mr);
    Answer A; A.groups = groups; A.ranked = n; A.rows.assign(nOut, 0xFFFFFFFFu); A.codes.assign(nOut, 0); A.sizes.assign(nOut, 0);
    for (uint32_t i = 0; i < n; i++) if (clp_emits(flag[i], pos[i], nOut)) { A.rows[pos[i]] = i; A.codes[pos[i]] = code[i]; A.sizes[pos[i]] = size[i]; }
    return A;
}
static Answer by_fold(const std::vector<uint32_t>& code, uint32_t keep, uint32_t mr) {
    const uint32_t n = (uint32_t)code.size();
    Answer A; A.ranked = n;
    std::set<uint32_t> seen(code.begin(), code.end()); A.groups = (uint32_t)seen.size();
    for (uint32_t i = 0; i < n && A.rows.size() < mr; i++) {
        uint32_t earlier = 0, all = 0;
        for (uint32_t j = 0; j < n; j++) if (code[j] == code[i]) { all++; if (j < i) earlier++; }
        if (earlier < keep) { A.rows.push_back(i); A.codes.push_back(code[i]); A.sizes.push_back(all); }
    }
    return A;
}
// value -> code: 0 and all ones are among the codes
static uint32_t code_of(uint32_t v) { return v == 0 ? 0u : v == 1 ? 0xFFFFFFFFu : v * 2654435761u; }

int main() {
    const uint32_t lengths[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024}, keeps[] = {1, 2, 3, 16};
    std::mt19937 rng(20240917u);
    unsigned long cases = 0;
    for (uint32_t n : lengths)
        for (int layout = 0; layout < 7; layout++) {
            std::vector<uint32_t> code(n);
            const uint32_t nrandom = layout == 4 ? 3 : layout == 5 ? 50 : 4096;
            for (uint32_t i = 0; i < n; i++) {
                uint32_t v = 0;
                if (layout == 0) v = 1;                                       // one group
                else if (layout == 1) v = n - 1 - i;                          // all distinct, descending values
                else if (layout == 2) v = i & 1;                              // two, alternating
                else if (layout == 3) v = i < (n + 1) / 2 ? 7 : i;            // one giant group first, then singletons
                else v = rng() % nrandom;
                code[i] = code_of(v);
            }
            for (uint32_t keep : keeps) {
                const uint32_t mrs[] = {1, 10, 64, n};
                for (uint32_t mr : mrs) {
                    const Answer a = by_steps(code, keep, mr), b = by_fold(code, keep, mr);
                    if (a.rows != b.rows || a.codes != b.codes || a.sizes != b.sizes || a.groups != b.groups || a.ranked != b.ranked) {
                        printf("MISMATCH n=%u layout=%d keep=%u mr=%u: %zu rows against %zu, %u groups against %u\n", n, layout, keep, mr, a.rows.size(), b.rows.size(), a.groups, b.groups);
                        return 1;
                    }
                    cases++;
                }
            }
        }
    printf("OK %lu\n", cases);
    return 0;
}
