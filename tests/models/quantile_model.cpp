// Host model of field_quantiles' selection: infidex_amd/csrc/quantile_select.h, listing_select.h and set_walk.h, UNCHANGED, driven serially the way
// k_quant_hist and k_quant_pick drive them (histogram -> pick -> histogram -> ...) for every (slot, quantile) at once over generated document sets, and
// compared target for target with a plain sort of each slot's keys.  tests/test_quantile_model.py compiles and runs it.
//   quantile_model            runs every case, prints "OK <selects> <targets> <targets of a slot that part at the last digit> <empty slots> <one-member slots>"
//                             or the first mismatch (exit 1)
//   quantile_model pos        reads "count q-as-its-64-bits" pairs from the standard input, prints qs_position of each
#define LS_FN static inline
#define SW_FN static inline
#include "quantile_select.h"
#include "set_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned long long u64;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }

static u64 g_selects = 0, g_targets = 0, g_lastDigit = 0, g_empty = 0, g_single = 0;

// One request.  rank / group / mask: heap blocks of exactly n elements (the walk may read nothing beyond them).  The whole set is the slot behind the groups.
struct Case {
    int32_t n; const uint32_t* rank; const uint32_t* group; const uint8_t* mask;
    uint32_t nvals, gvals, nanRanks, nq; const double* q; uint32_t db, lanes;
};

static bool fail(const char* what, const Case& C, uint32_t slot, uint32_t t) {
    printf("FAIL %s: n %d nvals %u gvals %u nq %u bits %u lanes %u slot %u target %u\n", what, C.n, C.nvals, C.gvals, C.nq, C.db, C.lanes, slot, t);
    return false;
}

static bool select_all(const Case& C) {
    const uint32_t w = C.db, nb = 1u << w, passes = ls_passes(C.nvals, w), slots = C.gvals + 1u, whole = slots - 1u;
    std::vector<ls_target> tgt((size_t)slots * C.nq); std::vector<uint32_t> count(slots, 0), nan(slots, 0);
    std::vector<uint32_t> partedAt((size_t)slots, passes);
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = ls_shift(p, passes, w), sw = qs_slot_words(p, C.nq, w);
        std::vector<uint32_t> tab((size_t)slots * sw, 0u);
        for (int64_t d0 = 0; d0 < C.n; d0 += SW_GROUP) {                       // k_quant_hist: a thread's 16 documents
            uint32_t m[4], rr[SW_GROUP], gc[SW_GROUP];
            sw_flags16(C.mask, C.n, d0, m);
            if (!sw_codes16(C.rank, C.n, d0, m, rr)) continue;
            if (C.group) sw_codes16(C.group, C.n, d0, m, gc);
            for (int j = 0; j < SW_GROUP; j++) {
                if (!sw_member(m, j) || rr[j] >= C.nvals) continue;
                const uint32_t k = qs_key(rr[j], C.nanRanks);
                const bool grouped = C.group && gc[j] < C.gvals;
                uint32_t at[2] = {whole, grouped ? gc[j] : whole};
                for (int x = 0; x < (grouped ? 2 : 1); x++) {
                    const uint32_t s = at[x];
                    if (p == 0) tab[(size_t)s * sw + (k ? ls_digit(k, shift, w) : nb)]++;
                    else if (k)
                        for (uint32_t t = 0; t < C.nq; t++)
                            if (ls_under_prefix(k, tgt[(size_t)s * C.nq + t].prefix, shift, w)) tab[(((size_t)s * C.nq + t) << w) + ls_digit(k, shift, w)]++;
                }
            }
        }
        const uint32_t per = (nb + C.lanes - 1) / C.lanes;                      // k_quant_pick: a lane's part of the row
        for (uint32_t s = 0; s < slots; s++)
            for (uint32_t t = 0; t < C.nq; t++) {
                const uint32_t* row = tab.data() + (p ? ((size_t)s * C.nq + t) << w : (size_t)s * sw);
                if (p == 0) { count[s] = 0; for (uint32_t b = 0; b < nb; b++) count[s] += row[b]; nan[s] = row[nb]; }
                const ls_target cur = p ? tgt[(size_t)s * C.nq + t] : qs_start(count[s], C.q[t]);
                ls_target next; next.prefix = QS_DEAD; next.resid = 0; uint32_t owners = 0, excl = 0;
                for (uint32_t lane = 0; lane < C.lanes; lane++) {
                    const uint32_t b0 = std::min(lane * per, nb), b1 = std::min(b0 + per, nb);
                    ls_target out;
                    if (qs_step(cur, row + b0, b0, b1 - b0, excl, w, &out)) { next = out; owners++; }
                    for (uint32_t b = b0; b < b1; b++) excl += row[b];
                }
                if (owners != (count[s] ? 1u : 0u)) return fail("a target's position must lie in exactly one part of its row", C, s, t);
                tgt[(size_t)s * C.nq + t] = next;
            }
        for (uint32_t s = 0; s < slots; s++)
            for (uint32_t t = 1; t < C.nq; t++)
                if (partedAt[s] == passes && tgt[(size_t)s * C.nq + t].prefix != tgt[(size_t)s * C.nq].prefix) partedAt[s] = p;
    }
    // the definition: a plain sort of every slot's keys
    std::vector<std::vector<uint32_t>> keys(slots); std::vector<uint32_t> nans(slots, 0);
    for (int32_t d = 0; d < C.n; d++) {
        if ((C.mask && C.mask[d]) || C.rank[d] >= C.nvals) continue;
        const bool grouped = C.group && C.group[d] < C.gvals;
        for (int x = 0; x < (grouped ? 2 : 1); x++) {
            const uint32_t s = x ? C.group[d] : whole;
            if (C.rank[d] < C.nanRanks) nans[s]++; else keys[s].push_back(C.rank[d]);
        }
    }
    for (uint32_t s = 0; s < slots; s++) {
        std::sort(keys[s].begin(), keys[s].end());
        if (count[s] != keys[s].size() || nan[s] != nans[s]) return fail("count or nan", C, s, 0);
        if (keys[s].empty()) g_empty++;
        if (keys[s].size() == 1) g_single++;
        if (passes > 1 && partedAt[s] == passes - 1) g_lastDigit++;
        for (uint32_t t = 0; t < C.nq; t++) {
            const uint32_t got = qs_rank(tgt[(size_t)s * C.nq + t]);
            if (keys[s].empty()) { if (got != QS_DEAD) return fail("an empty slot answered", C, s, t); continue; }
            volatile double x = (double)(keys[s].size() - 1) * C.q[t];
            const size_t pos = (size_t)std::floor(x);
            if (pos >= keys[s].size() || got != keys[s][pos]) return fail("rank", C, s, t);
            g_targets++;
        }
    }
    g_selects++;
    return true;
}

// kind 0: random ranks; 1: all equal; 2: two values that differ in the last digit only (and their neighbours); 3: ranks near the top of the range
static bool run(int32_t n, uint32_t nvals, uint32_t gvals, uint32_t nanRanks, int kind, int maskKind, const std::vector<double>& q, uint32_t db, uint32_t lanes) {
    uint32_t* rank = (uint32_t*)malloc((size_t)n * 4); uint32_t* group = gvals ? (uint32_t*)malloc((size_t)n * 4) : nullptr; uint8_t* mask = maskKind ? (uint8_t*)malloc((size_t)n) : nullptr;
    const uint32_t base = nvals > 40 ? (rnd() % (nvals - 32)) & ~15u : 0u, same = rnd() % nvals;
    for (int32_t d = 0; d < n; d++) {
        uint32_t r = rnd() % nvals;
        if (kind == 1) r = same;
        if (kind == 2) r = std::min(nvals - 1u, base + (rnd() & 1u) + (rnd() % 16 == 0 ? 2u : 0u));
        if (kind == 3) r = nvals - 1u - rnd() % std::min(nvals, 5u);
        if (nanRanks && rnd() % 5 == 0) r = 0;
        rank[d] = r;
        if (group) group[d] = rnd() % (gvals + (gvals > 3 ? 2u : 0u));      // (codes at or beyond gvals belong to no group; some groups stay empty)
        if (mask) mask[d] = maskKind == 2 ? (d == n - 1 ? 0 : 1) : (maskKind == 3 ? 1 : (rnd() % 3 == 0 ? (uint8_t)(1 + rnd() % 255) : 0));
    }
    if (group && gvals > 2) for (int32_t d = 0; d < n; d++) if (group[d] == 1) group[d] = 0;      // group 1 is always empty
    Case C = {n, rank, group, mask, nvals, gvals, nanRanks, (uint32_t)q.size(), q.data(), db, lanes};
    const bool ok = select_all(C);
    free(rank); free(group); free(mask);
    return ok;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "pos")) {
        unsigned c; u64 bits;
        while (scanf("%u %llu", &c, &bits) == 2) { double q; memcpy(&q, &bits, 8); printf("%u\n", qs_position(c, q)); }
        return 0;
    }
    const std::vector<std::vector<double>> qsets = {
        {0.5}, {0.0, 1.0}, {0.0, 0.25, 0.5, 0.75, 1.0},
        {0.9, 0.1, 0.5, 0.5, 1.0 / 3, 0.999, 0.0, 1.0, 0.75, 0.25, 0.1, 0.95, 0.05, 0.5, 1.0, 0.0}, {0.5, 0.5000001, 0.51}};
    // every digit width, nvals around every power of two where the number of passes changes for some width, document counts around the walk's groups
    for (uint32_t db = LS_MIN_DIGIT_BITS; db <= LS_MAX_DIGIT_BITS; db++) {
        for (uint32_t k = 1; k <= 24; k += (k < 13 ? 1 : 5)) {
            for (int dv = -2; dv <= 1; dv++) {
                const uint32_t nvals = (uint32_t)((int64_t)(1u << k) + dv);
                if (!nvals) continue;
                // the select's bits are those of nvals + 1 (listing_select.h): 2^k - 2 values are the last to take k bits, 2^k - 1 the first to take k + 1
                for (int kind = 0; kind < 4; kind++) {
                    const int32_t n = (int32_t)(1 + rnd() % 700);
                    const std::vector<double>& q = qsets[(k + kind + db) % qsets.size()];
                    if (!run(n, nvals, kind == 0 ? 0 : (kind == 1 ? 7 : 40), (k + kind) % 3 == 0 ? 1u : 0u, kind, (int)(rnd() % 2), q, db, (db + k) % 2 ? 64u : 1u)) return 1;
                }
            }
        }
        // the pass count really changes there: between 2^k - 2 and 2^k - 1 values, k a multiple of the width
        for (uint32_t k = db; k <= 3 * db && k < 32; k += db) {
            const uint32_t a = ls_passes((1u << k) - 2u, db), b = ls_passes((1u << k) - 1u, db);
            if (a != k / db || b != a + 1 || ls_passes(1u << k, db) != b || ls_passes((1u << k) + 1u, db) != b) { printf("FAIL passes at 2^%u, %u bits\n", k, db); return 1; }
        }
        // keys up to 31 bits
        for (int kind = 0; kind < 4; kind++)
            if (!run(300, 0x7FFFFFFEu, kind & 1 ? 5 : 0, 0, kind, 1, qsets[3], db, 64)) return 1;
        // small sets: one member (alone, behind a mask that leaves the last document only), twelve to thirty-three documents, a mask that accepts nothing
        for (int32_t n : {1, 2, 12, 15, 16, 17, 31, 32, 33})
            for (int mk = 0; mk < 4; mk++)
                for (size_t qi = 0; qi < qsets.size(); qi++)
                    if (!run(n, 1000, mk == 1 ? 3 : 0, mk == 0 ? 1 : 0, qi % 2 ? 2 : 0, mk, qsets[qi], db, 64)) return 1;
    }
    if (!g_lastDigit || !g_empty || !g_single) { printf("FAIL a case was never met: last-digit %llu empty %llu single %llu\n", g_lastDigit, g_empty, g_single); return 1; }
    printf("OK %llu %llu %llu %llu %llu\n", g_selects, g_targets, g_lastDigit, g_empty, g_single);
    return 0;
}
